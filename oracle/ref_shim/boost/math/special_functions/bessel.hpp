/*
 * oracle/ref_shim/boost/math/special_functions/bessel.hpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Stand-in for the one Boost function the reference calls.  Boost is not vendored in the reference and
 * is not required to build this project, so boost::math::cyl_bessel_k forwards to the oracle's own
 * K_nu (oracle/cocons_oracle.c, pinned by tests/golden/besselk_grid.json against 40-digit mpmath).
 * The compiled reference therefore pins everything AROUND K_nu, not K_nu itself.
 */
#ifndef COCONS_REF_SHIM_BOOST_BESSEL_HPP
#define COCONS_REF_SHIM_BOOST_BESSEL_HPP

extern "C" double oracle_besselk(double nu, double x);

namespace boost {
namespace math {

inline double cyl_bessel_k(double v, double x) { return oracle_besselk(v, x); }

}  // namespace math
}  // namespace boost

#endif
