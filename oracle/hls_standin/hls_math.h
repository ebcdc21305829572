/*
 * hls_math.h -- stand-in for the Vitis HLS header (own text; see ap_fixed.h).
 *
 * Float form: <cmath> in fp32.
 *
 * Fixed form: exactly the rules R3-R6 of oracle/q_oracle.c, on the argument's own grid (F fractional bits, W bits,
 * "pattern" = the two's-complement integer).  These four rules are a reading of Vitis, not a run of it; running the
 * reference against this header pins the program around them, not the rules themselves.
 *   R3  sqrt(x)  = isqrt(pattern << F) for pattern > 0, else 0
 *   R4  recip(x) = floor(2^(2F) / pattern) for pattern > 0, else 0
 *   R5  exp(x), log(x) = the real function evaluated in double precision, floored to the grid and wrapped;
 *       an exp too large for 64 bits gives 0, log(x <= 0) = 0
 *   R6  abs(x)   = |pattern| wrapped (the most negative pattern is its own abs)
 * signbit(x) is the pattern's sign in both forms (fp32: the sign bit, so -0.0f counts as negative).
 */
#ifndef HLS_STANDIN_HLS_MATH_H
#define HLS_STANDIN_HLS_MATH_H

#include <cmath>
#include "ap_fixed.h"

namespace hls {
#ifndef HLS_STANDIN_FIXED
template <int W, int I> bool signbit(const ap_fixed<W, I>& x) { return std::signbit(x.v); }
template <int W, int I> ap_fixed<W, I> sqrt(const ap_fixed<W, I>& x) { return ap_fixed<W, I>(std::sqrt(x.v)); }
template <int W, int I> ap_fixed<W, I> recip(const ap_fixed<W, I>& x) { return ap_fixed<W, I>(1.0f / x.v); }
template <int W, int I> ap_fixed<W, I> exp(const ap_fixed<W, I>& x) { return ap_fixed<W, I>(std::exp(x.v)); }
template <int W, int I> ap_fixed<W, I> log(const ap_fixed<W, I>& x) { return ap_fixed<W, I>(std::log(x.v)); }
template <int W, int I> ap_fixed<W, I> abs(const ap_fixed<W, I>& x) { return ap_fixed<W, I>(std::fabs(x.v)); }
#else
namespace standin_detail {
inline unsigned long long isqrt(unsigned __int128 x)
{
    unsigned long long r = (unsigned long long)std::sqrt((double)x);
    while ((unsigned __int128)r * r > x) r--;
    while ((unsigned __int128)(r + 1) * (r + 1) <= x) r++;
    return r;
}
}  // namespace standin_detail
template <int W, int I> bool signbit(const ap_fixed<W, I>& x) { return x.pattern() < 0; }
template <int W, int I> ap_fixed<W, I> sqrt(const ap_fixed<W, I>& x) /* R3 */
{
    static_assert(W + (W - I) <= 120, "hls::sqrt stand-in: argument too wide");
    if (x.pattern() <= 0) return ap_fixed<W, I>::from_pattern(0);
    return ap_fixed<W, I>::from_pattern((hls_standin::wide_t)standin_detail::isqrt((unsigned __int128)x.pattern() << (W - I)));
}
template <int W, int I> ap_fixed<W, I> recip(const ap_fixed<W, I>& x) /* R4 */
{
    static_assert(2 * (W - I) <= 120, "hls::recip stand-in: argument too wide");
    if (x.pattern() <= 0) return ap_fixed<W, I>::from_pattern(0);
    return ap_fixed<W, I>::from_pattern(((hls_standin::wide_t)1 << (2 * (W - I))) / x.pattern());
}
template <int W, int I> ap_fixed<W, I> exp(const ap_fixed<W, I>& x) /* R5 */
{
    static_assert(W < 54, "hls::exp stand-in: argument too wide for double");
    double v = std::floor(std::ldexp(std::exp(x.to_double()), W - I));
    return ap_fixed<W, I>::from_pattern(v >= 9.0e18 ? 0 : (hls_standin::wide_t)(long long)v);
}
template <int W, int I> ap_fixed<W, I> log(const ap_fixed<W, I>& x) /* R5 */
{
    static_assert(W < 54, "hls::log stand-in: argument too wide for double");
    if (x.pattern() <= 0) return ap_fixed<W, I>::from_pattern(0);
    return ap_fixed<W, I>::from_pattern((hls_standin::wide_t)(long long)std::floor(std::ldexp(std::log(x.to_double()), W - I)));
}
template <int W, int I> ap_fixed<W, I> abs(const ap_fixed<W, I>& x) /* R6 */
{
    return ap_fixed<W, I>::from_pattern(x.pattern() < 0 ? -x.pattern() : x.pattern());
}
#endif
}  // namespace hls
#endif
