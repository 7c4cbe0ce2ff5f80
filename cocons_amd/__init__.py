"""cocons_amd -- MI355X-native dense hot path of the R package blasif/cocons.

Host-side mirror of the reference's operator interface for this path (same
names and argument meaning as the R functions) over the C ABI in
include/cocons_hip.h.  See DESIGN.md / INTEGRATION.md.
"""
from .host import (  # noqa: F401
    ASPECTS,
    CoconsFit,
    CoconsTaperFit,
    GetNeg2loglikelihood,
    GetNeg2loglikelihoodTaper,
    GetNeg2loglikelihoodTaperProfile,
    GetNeg2loglikelihoodTaperProfile_grad,
    GetNeg2loglikelihoodTaper_grad,
    GetNeg2loglikelihoodProfile,
    GetNeg2loglikelihoodREML,
    GetNeg2loglikelihoodProfile_grad,
    GetNeg2loglikelihoodREML_grad,
    GetNeg2loglikelihood_batch,
    GetNeg2loglikelihood_grad,
    cocoCV_dense,
    cocoCV_sparse,
    cocoPredict_dense,
    cocoPredict_dense_chunked,
    cocoPredict_sparse,
    cocoSim_cond_dense,
    cocoSim_dense,
    cocoSim_sparse,
    cov_rns,
    cov_rns_classic,
    cov_rns_pred,
    cov_rns_taper,
    cov_rns_taper_pred,
    getBetas_profile,
    getCRPS,
    getFisher_dense,
    getFisher_reml,
    getHessian_dense,
    getLogScore,
    getModelLists,
    getModelLists_grad,
    getPen,
    getPen_grad,
    getScale,
    sumsmoothlone,
)
from ._lib import CholeskyError, CoconsHipError  # noqa: F401
