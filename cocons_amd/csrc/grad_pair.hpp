// grad_pair.hpp -- the pair partials every analytic gradient contracts: the Matern correlation with its u- and
// nu-derivatives, and the partials of one covariance entry with respect to the site predictors of both sides and the global
// range.  Shared by grad.hip (dense gradient, Fisher information: a global SoA) and vecchia.hip (the block gradient: the
// block's parameters in LDS); both read through a pointer and a stride, as pair_value_idx does.
// Compile with -ffp-contract=off (matern_device.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include "matern_device.hpp"

namespace cocons {

constexpr int GFAM = 6;            // site families: std.dev, scale, aniso, tilt, smooth, nugget (theta's row order)
constexpr int TH_SD_ = 0, TH_SCALE_ = 1, TH_NG_ = 5;

// ---------------------------------------------------------------------------
// 2^(1-nu)/Gamma(nu) u^nu K_nu(u) and its u-derivative -2^(1-nu)/Gamma(nu) u^nu K_{nu-1}(u), 0 < u < 706, nu > 0.
// Temme's series (u <= 2) or Steed's CF2 (u > 2) give K_mu, K_{mu+1} with mu = nu - round(nu); the forward recurrence
// up to order nu keeps the order below it (matern_bessel's scheme, with the neighbouring order kept).  nu < 1/2 (n = 0) needs
// K_{nu-1} = K_{1-mu}: both schemes give it directly, as the neighbour K_{(-mu)+1} of K_{-mu} = K_mu (Temme's sum with q in the
// place of p; the continued fraction's ratio at -mu).  K_{mu+1} - (2 mu / u) K_mu is the same number, but its two terms agree
// to leading order at small u and leave a relative error of eps (2 / u)^(2 nu): 3e-6 at nu -> 1/2, u = 1e-10.
static __device__ __noinline__ void matern_pair(double nu, double u, double &M, double &Mu)
{
    const double tol = 2.220446049250313e-16;
    const double pi = 3.14159265358979323846;
    const int n = (int)floor(nu + 0.5);
    const double mu = nu - n, mu2 = mu * mu;
    double gam1 = 0.0, gam2 = 0.0;
    for (int j = RG_NTERMS - 1; j >= 0; --j) {
        gam1 = fma(gam1, mu2, c_rg_odd[j]);
        gam2 = fma(gam2, mu2, c_rg_even[j]);
    }
    const double gampl = gam2 - mu * gam1;   // 1/Gamma(1+mu)
    const double gammi = gam2 + mu * gam1;   // 1/Gamma(1-mu)
    double kmu, kmu1;
    bool scaled;                             // K values carry the factor e^u (CF2)
    if (u <= 2.0) {
        const double x2 = 0.5 * u, pimu = pi * mu;
        const double fact = fabs(pimu) < tol ? 1.0 : pimu / sin(pimu);
        double d = -log(x2);
        double e = mu * d;
        const double fact2 = fabs(e) < tol ? 1.0 : sinh(e) / e;
        double ff = fact * (gam1 * cosh(e) + gam2 * fact2 * d);
        double sum = ff;
        e = exp(e);
        double pp = 0.5 * e / gampl, q = 0.5 / (e * gammi), c = 1.0;
        d = x2 * x2;
        double sum1 = (n == 0) ? q : pp;
        for (int i = 1; i < 500; ++i) {
            const double di = (double)i;
            ff = (di * ff + pp + q) / ((di - mu) * (di + mu));
            c *= d / di;
            pp /= (di - mu);
            q /= (di + mu);
            const double del = c * ff;
            sum += del;
            sum1 += c * (((n == 0) ? q : pp) - di * ff);
            if (fabs(del) < fabs(sum) * tol) break;
        }
        kmu = sum;
        kmu1 = sum1 * (2.0 / u);
        scaled = false;
    } else {
        double a = mu2 - 0.25;
        double b = 2.0 * (u + 1.0), D = 1.0 / b, f = D, delta = D;
        double Ak = -a, Bk = 0.0;
        double Q = Ak, S = 1.0 + Q * delta;
        for (int k = 2; k < 500; ++k) {
            a -= 2 * (k - 1);
            b += 2.0;
            D = 1.0 / (a * D + b);
            delta *= b * D - 1.0;
            f += delta;
            const double An = -(Bk - (b - 2.0) * Ak) / (double)k;
            Bk = -(a / (double)k) * Ak;
            Ak = An;
            Q += Ak;
            const double qd = Q * delta;
            S += qd;
            if (fabs(qd) < fabs(S) * tol) break;
        }
        kmu = sqrt(pi / (2.0 * u)) / S;
        kmu1 = kmu * (0.5 + ((n == 0) ? -mu : mu) + u + (mu2 - 0.25) * f) / u;
        scaled = true;
    }
    // K_{nu-1}, K_nu: n >= 1 keeps the order below nu from the recurrence; n = 0 has K_{1-mu} = K_{mu-1} in kmu1
    double klo = kmu1, khi = kmu;
    if (n >= 1) { klo = kmu; khi = kmu1; }
    for (int k = 1; k < n; ++k) {
        const double next = (2.0 * (mu + k) / u) * khi + klo;
        klo = khi;
        khi = next;
    }
    double prod = 1.0;
    for (int k = 1; k < n; ++k) prod *= (mu + k);
    const double rg = ((n == 0) ? mu * gampl : gampl) / prod;      // 1/Gamma(nu)
    const double ex = nu * log2(u) + 1.0 - nu;
    const double pre = (scaled ? pow2a_expmu(ex, u) : exp2(ex)) * rg;
    M = pre * khi;
    Mu = -pre * klo;
}

// dM/dnu at fixed u: four-point central difference (step 1e-3 nu: truncation ~1e-11 relative, rounding ~1e-12)
static __device__ double matern_dnu(double nu, double u)
{
    const double h = 1e-3 * nu;
    double m1, m2, m3, m4, t;
    matern_pair(nu + h, u, m1, t);
    matern_pair(nu - h, u, m2, t);
    matern_pair(nu + 2 * h, u, m3, t);
    matern_pair(nu - 2 * h, u, m4, t);
    return (8.0 * (m1 - m2) - (m3 - m4)) / (12.0 * h);
}

// ---------------------------------------------------------------------------
// Partials of one off-diagonal entry C(ii = ia, jj = ib) with respect to the site predictors of both sides and the global
// range, branch for branch as pair_value_idx evaluates it (pair_sym_kernel: u <= eps gives the ii site's diagonal).
// L: loc_params_kernel's fields, field f of location i at L[f sl + i]; G: launch_grad_site's (GSITE_FIELDS), at G[f sg + i].
template <int MODE>
__device__ __forceinline__ void pair_partials(const double *L, size_t sl, const double *G, size_t sg, double gr, double nu_fixed,
                                              int smooth_free, int ia, int ib, double da[GFAM], double db[GFAM], double &dglob)
{
    const double eps = 2.220446049250313e-16;
#define LF(f, i) L[(size_t)(f) * sl + (i)]
#define GF(f, i) G[(size_t)(f) * sg + (i)]
    for (int f = 0; f < GFAM; ++f) { da[f] = 0.0; db[f] = 0.0; }
    dglob = 0.0;
    const double rda = LF(2, ia), an2a = LF(3, ia), raa = LF(4, ia), cta = LF(5, ia), sta = LF(6, ia);
    const double rdb = LF(2, ib), an2b = LF(3, ib), rab = LF(4, ib), ctb = LF(5, ib), stb = LF(6, ib);
    const double s11 = 0.5 * (rda + rdb), s22 = 0.5 * (rda * an2a + rdb * an2b), s12 = 0.5 * (raa * cta + rab * ctb);
    const double D = s11 * s22 - s12 * s12;
    const double dx = LF(0, ia) - LF(0, ib), dy = LF(1, ia) - LF(1, ib);
    const double dxx = dx * dx, dyy = dy * dy, dxy = dx * dy;
    const double q = s22 * dxx + s11 * dyy - 2.0 * s12 * dxy;
    const double nu = (MODE == MODE_GEOM) ? LF(10, ia) * LF(10, ib) : nu_fixed;
    const double u = sqrt(8.0 * nu * q / (gr * D));
    if (u <= eps) {                       // coincident: C = exp(eta_sd) + ng of the ii site alone
        da[TH_SD_] = GF(3, ia);
        da[TH_NG_] = LF(12, ia);
        return;
    }
    if (u >= 706.0) return;               // the reference's stand-in: rounds to 0
    double M, Mu, Mn = 0.0;
    if (MODE == MODE_HALF) { M = exp(-u); Mu = -M; }
    else if (MODE == MODE_THREEHALF) { const double e = exp(-u); M = (1.0 + u) * e; Mu = -u * e; }
    else if (MODE == MODE_FIVEHALF) { const double e = exp(-u); M = (1.0 + u + u * u / 3.0) * e; Mu = -(u / 3.0) * (1.0 + u) * e; }
    else {
        matern_pair(nu, u, M, Mu);
        if (smooth_free) Mn = matern_dnu(nu, u);
    }
    const double P = LF(9, ia) * LF(9, ib) * sqrt(LF(8, ia) * LF(8, ib) / D);
    const double C = M * P, U = P * Mu * u;                 // U = dC / dlog u
    dglob = -U;                                             // gr = e^(2 theta_scale,0): dlog u = -1
    auto side = [&](int i, double rd, double an2, double ra, double ct, double st, double *d) {
        const double tp = GF(0, i), cot = GF(1, i);
        // (s11', s22', s12') of the three geometric predictors, then dlog u = (q'/q - D'/D) / 2 and the amplitude's
        // dlog = dlog(rd a sin t) / 2 - D'/(2 D)
        const double s11p[3] = {0.5 * rd, 0.0, 0.0};
        const double s22p[3] = {0.5 * rd * an2, rd * an2, 0.0};
        const double s12p[3] = {0.5 * ra * ct, 0.5 * ra * ct, -0.5 * ra * st * tp};
        const double amp[3] = {0.5, 0.5, 0.5 * cot * tp};
        for (int k = 0; k < 3; ++k) {
            const double Dp = s11p[k] * s22 + s11 * s22p[k] - 2.0 * s12 * s12p[k];
            const double qp = s22p[k] * dxx + s11p[k] * dyy - 2.0 * s12p[k] * dxy;
            const double dlu = 0.5 * (qp / q - Dp / D);
            const double dlp = amp[k] - 0.5 * Dp / D;
            d[1 + k] = U * dlu + C * dlp;
        }
        d[TH_SD_] = 0.5 * C;
        if (smooth_free) {
            const double dl = GF(2, i);                        // dlog nu_ij
            d[4] = P * Mn * nu * dl + U * 0.5 * dl;
        }
    };
    side(ia, rda, an2a, raa, cta, sta, da);
    side(ib, rdb, an2b, rab, ctb, stb, db);
#undef LF
#undef GF
}

}  // namespace cocons
