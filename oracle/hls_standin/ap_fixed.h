/*
 * ap_fixed.h -- stand-in for the Vitis HLS header of the same name, written for this project from the published
 * semantics of ap_fixed (no text of Vitis or of the reference).  TEST INFRASTRUCTURE: it exists so that the
 * reference's kernel sources compile unchanged on a CPU and can be run beside the oracle's C files (make -C oracle ref).
 *
 * Two forms:
 *
 *   float form (default): ap_fixed<W,I> holds one float and every operator is the fp32 operator.  This runs the
 *       reference's program in fp32 and pins the float oracles.
 *
 *   fixed form (-DHLS_STANDIN_FIXED): ap_fixed<W,I> is a W-bit two's-complement pattern with I integer bits and
 *       F = W - I fractional bits, quantisation AP_TRN (floor on store) and overflow AP_WRAP (keep the low W bits),
 *       the published defaults.  An expression is exact until it is stored:
 *           a + b, a - b   one more integer bit than the larger, the larger fraction
 *           a * b          W1 + W2 bits, I1 + I2 integer bits
 *           a / b          F_a + I_b fractional bits (I_a + F_b + 1 integer bits), integer divide toward zero
 *           -a             one more integer bit
 *           int operand    ap_fixed<32,32>
 *           from double    floor to the grid, wrap
 *       Compound assignment computes the wide result and stores it.
 *
 * Choices the published semantics leave open, all made here (DESIGN.md section 2 lists them):
 *   C1  a / b with b == 0 gives 0, in both forms.  ap_fixed publishes no result for it, and the reference's own text counts
 *       on this one: PNA/src/node_embedding.cc:149-150 computes avg_deg / log_degree and then tests the quotient for 0,
 *       which only a zero log_degree (a node without out-edges) can produce.  Under IEEE division the fp32 program would
 *       instead carry inf / NaN into a sign test (DGN/src/node_embedding.cc:143,177).
 *   C2  comparison with a floating literal (== 0.0) converts the ap_fixed operand to double, which is exact for every
 *       width below 54 bits, and compares doubles.
 *   C3  construction from float goes through double (exact), then as from double.
 *   C4  a non-finite double constructs 0.
 *   C6  to_int() truncates toward zero, as the C conversion of a double does (the reference's kernels never call it).
 *   C5  intermediate widths are capped by the 128-bit carrier: wider is a compile-time error, never a silent wrap.
 */
#ifndef HLS_STANDIN_AP_FIXED_H
#define HLS_STANDIN_AP_FIXED_H

#include <cmath>
#include <cstdint>

#ifndef HLS_STANDIN_FIXED

/* ------------------------------------------------------------------------------------------------- float form */
template <int W, int I>
struct ap_fixed {
    static constexpr int width = W;
    static constexpr int iwidth = I;
    float v;
    ap_fixed() = default;
    constexpr ap_fixed(float x) : v(x) {}
    constexpr ap_fixed(double x) : v((float)x) {}
    constexpr ap_fixed(int x) : v((float)x) {}
    template <int W2, int I2>
    constexpr ap_fixed(const ap_fixed<W2, I2>& o) : v(o.v) {}
    float to_float() const { return v; }
    double to_double() const { return (double)v; }
    int to_int() const { return (int)v; }
    constexpr ap_fixed operator-() const { return ap_fixed(-v); }
    template <typename T> ap_fixed& operator+=(const T& o) { *this = *this + o; return *this; }
    template <typename T> ap_fixed& operator-=(const T& o) { *this = *this - o; return *this; }
    template <typename T> ap_fixed& operator*=(const T& o) { *this = *this * o; return *this; }
    template <typename T> ap_fixed& operator/=(const T& o) { *this = *this / o; return *this; }
};

#define HLS_STANDIN_BINOP(op)                                                                                         \
    template <int W, int I, int W2, int I2>                                                                           \
    constexpr ap_fixed<W, I> operator op(const ap_fixed<W, I>& a, const ap_fixed<W2, I2>& b) { return ap_fixed<W, I>(a.v op b.v); } \
    template <int W, int I>                                                                                           \
    constexpr ap_fixed<W, I> operator op(const ap_fixed<W, I>& a, int b) { return ap_fixed<W, I>(a.v op (float)b); }    \
    template <int W, int I>                                                                                           \
    constexpr ap_fixed<W, I> operator op(int a, const ap_fixed<W, I>& b) { return ap_fixed<W, I>((float)a op b.v); }
HLS_STANDIN_BINOP(+)
HLS_STANDIN_BINOP(-)
HLS_STANDIN_BINOP(*)
#undef HLS_STANDIN_BINOP
/* C1: x / 0 = 0, as in the fixed form */
constexpr float hls_standin_fdiv(float a, float b) { return b == 0.0f ? 0.0f : a / b; }
template <int W, int I, int W2, int I2>
constexpr ap_fixed<W, I> operator/(const ap_fixed<W, I>& a, const ap_fixed<W2, I2>& b) { return ap_fixed<W, I>(hls_standin_fdiv(a.v, b.v)); }
template <int W, int I>
constexpr ap_fixed<W, I> operator/(const ap_fixed<W, I>& a, int b) { return ap_fixed<W, I>(hls_standin_fdiv(a.v, (float)b)); }
template <int W, int I>
constexpr ap_fixed<W, I> operator/(int a, const ap_fixed<W, I>& b) { return ap_fixed<W, I>(hls_standin_fdiv((float)a, b.v)); }

#define HLS_STANDIN_CMP(op)                                                                                           \
    template <int W, int I, int W2, int I2>                                                                           \
    constexpr bool operator op(const ap_fixed<W, I>& a, const ap_fixed<W2, I2>& b) { return a.v op b.v; }             \
    template <int W, int I> constexpr bool operator op(const ap_fixed<W, I>& a, int b) { return a.v op (float)b; }      \
    template <int W, int I> constexpr bool operator op(int a, const ap_fixed<W, I>& b) { return (float)a op b.v; }      \
    template <int W, int I> constexpr bool operator op(const ap_fixed<W, I>& a, double b) { return (double)a.v op b; }  \
    template <int W, int I> constexpr bool operator op(double a, const ap_fixed<W, I>& b) { return a op (double)b.v; }
HLS_STANDIN_CMP(==)
HLS_STANDIN_CMP(!=)
HLS_STANDIN_CMP(<)
HLS_STANDIN_CMP(<=)
HLS_STANDIN_CMP(>)
HLS_STANDIN_CMP(>=)
#undef HLS_STANDIN_CMP

#else /* HLS_STANDIN_FIXED */

/* ------------------------------------------------------------------------------------------------- fixed form */
namespace hls_standin {
typedef __int128 wide_t;
typedef unsigned __int128 uwide_t;
constexpr int kCarrierBits = 120; /* C5 */

template <bool le16, bool le32, bool le64> struct pick { typedef wide_t type; };
template <> struct pick<true, true, true> { typedef int16_t type; };
template <> struct pick<false, true, true> { typedef int32_t type; };
template <> struct pick<false, false, true> { typedef int64_t type; };

constexpr int imax(int a, int b) { return a > b ? a : b; }

/* x * 2^k without shifting a negative value left */
constexpr wide_t shl(wide_t x, int k) { return (wide_t)((uwide_t)x << k); }
/* keep the low W bits of x, sign-extended (AP_WRAP) */
constexpr wide_t wrap(wide_t x, int W) { return (wide_t)((uwide_t)x << (128 - W)) >> (128 - W); }
/* move a pattern with f_from fractional bits onto a grid with f_to: floor (AP_TRN) or exact */
constexpr wide_t regrid(wide_t x, int f_from, int f_to) { return f_from > f_to ? (x >> (f_from - f_to)) : shl(x, f_to - f_from); }
}  // namespace hls_standin

template <int W, int I>
struct ap_fixed {
    static_assert(W >= 1 && W <= hls_standin::kCarrierBits, "ap_fixed stand-in: width exceeds the 128-bit carrier (C5)");
    static constexpr int width = W;
    static constexpr int iwidth = I;
    static constexpr int F = W - I;
    typedef typename hls_standin::pick<(W <= 16), (W <= 32), (W <= 64)>::type store_t;
    store_t v; /* the pattern, sign-extended; arrays of ap_fixed<16,*> are arrays of int16_t */

    ap_fixed() = default;
    constexpr ap_fixed(int x) : v((store_t)hls_standin::wrap(hls_standin::regrid((hls_standin::wide_t)x, 0, F), W)) {}
    ap_fixed(double x) : v((store_t)from_double(x)) {}
    ap_fixed(float x) : v((store_t)from_double((double)x)) {} /* C3 */
    template <int W2, int I2>
    constexpr ap_fixed(const ap_fixed<W2, I2>& o)
        : v((store_t)hls_standin::wrap(hls_standin::regrid((hls_standin::wide_t)o.v, W2 - I2, F), W)) {}

    static constexpr ap_fixed from_pattern(hls_standin::wide_t p)
    {
        ap_fixed r(0);
        r.v = (store_t)hls_standin::wrap(p, W);
        return r;
    }
    static hls_standin::wide_t from_double(double x)
    {
        if (!std::isfinite(x)) return 0; /* C4 */
        double s = std::floor(std::ldexp(x, F));
        /* wrap: reduce mod 2^W in double (exact: s is an integer, fmod is exact), then to integer */
        double m = std::ldexp(1.0, W);
        double r = std::fmod(s, m);
        if (r < 0) r += m;
        static_assert(W <= 64, "ap_fixed stand-in: construction from double is for widths up to 64");
        hls_standin::uwide_t u = (hls_standin::uwide_t)(unsigned long long)r; /* 0 <= r < 2^W */
        return hls_standin::wrap((hls_standin::wide_t)u, W);
    }
    constexpr hls_standin::wide_t pattern() const { return (hls_standin::wide_t)v; }
    double to_double() const { return std::ldexp((double)v, -F); }
    float to_float() const { return (float)to_double(); }
    int to_int() const { return (int)(pattern() / ((hls_standin::wide_t)1 << F)); } /* C6: toward zero, as a C cast */

    constexpr ap_fixed<W + 1, I + 1> operator-() const { return ap_fixed<W + 1, I + 1>::from_pattern(-pattern()); }
    template <typename T> ap_fixed& operator+=(const T& o) { *this = ap_fixed(*this + o); return *this; }
    template <typename T> ap_fixed& operator-=(const T& o) { *this = ap_fixed(*this - o); return *this; }
    template <typename T> ap_fixed& operator*=(const T& o) { *this = ap_fixed(*this * o); return *this; }
    template <typename T> ap_fixed& operator/=(const T& o) { *this = ap_fixed(*this / o); return *this; }
};

namespace hls_standin {
template <int W1, int I1, int W2, int I2>
struct rt {
    static constexpr int F1 = W1 - I1, F2 = W2 - I2;
    static constexpr int sumF = imax(F1, F2), sumI = imax(I1, I2) + 1;
    typedef ap_fixed<sumI + sumF, sumI> sum;
    typedef ap_fixed<W1 + W2, I1 + I2> prod;
    static constexpr int divF = F1 + I2, divI = I1 + F2 + 1;
    typedef ap_fixed<divI + divF, divI> quot;
};
typedef ap_fixed<32, 32> int_t;
}  // namespace hls_standin

template <int W1, int I1, int W2, int I2>
constexpr typename hls_standin::rt<W1, I1, W2, I2>::sum operator+(const ap_fixed<W1, I1>& a, const ap_fixed<W2, I2>& b)
{
    typedef hls_standin::rt<W1, I1, W2, I2> R;
    return R::sum::from_pattern(hls_standin::regrid(a.pattern(), R::F1, R::sumF) + hls_standin::regrid(b.pattern(), R::F2, R::sumF));
}
template <int W1, int I1, int W2, int I2>
constexpr typename hls_standin::rt<W1, I1, W2, I2>::sum operator-(const ap_fixed<W1, I1>& a, const ap_fixed<W2, I2>& b)
{
    typedef hls_standin::rt<W1, I1, W2, I2> R;
    return R::sum::from_pattern(hls_standin::regrid(a.pattern(), R::F1, R::sumF) - hls_standin::regrid(b.pattern(), R::F2, R::sumF));
}
template <int W1, int I1, int W2, int I2>
constexpr typename hls_standin::rt<W1, I1, W2, I2>::prod operator*(const ap_fixed<W1, I1>& a, const ap_fixed<W2, I2>& b)
{
    return hls_standin::rt<W1, I1, W2, I2>::prod::from_pattern(a.pattern() * b.pattern());
}
template <int W1, int I1, int W2, int I2>
constexpr typename hls_standin::rt<W1, I1, W2, I2>::quot operator/(const ap_fixed<W1, I1>& a, const ap_fixed<W2, I2>& b)
{
    typedef hls_standin::rt<W1, I1, W2, I2> R;
    /* a = pa 2^-F1, b = pb 2^-F2: quotient pattern on the 2^-(F1 + I2) grid = trunc(pa 2^(F2 + I2) / pb) = trunc(pa 2^W2 / pb) */
    static_assert(W1 + W2 <= hls_standin::kCarrierBits, "ap_fixed stand-in: dividend exceeds the carrier (C5)");
    if (b.pattern() == 0) return R::quot::from_pattern(0); /* C1 */
    return R::quot::from_pattern(hls_standin::shl(a.pattern(), W2) / b.pattern());
}

#define HLS_STANDIN_INT_BINOP(op)                                                                                     \
    template <int W, int I> constexpr auto operator op(const ap_fixed<W, I>& a, int b) -> decltype(a op hls_standin::int_t(b)) { return a op hls_standin::int_t(b); } \
    template <int W, int I> constexpr auto operator op(int a, const ap_fixed<W, I>& b) -> decltype(hls_standin::int_t(a) op b) { return hls_standin::int_t(a) op b; }
HLS_STANDIN_INT_BINOP(+)
HLS_STANDIN_INT_BINOP(-)
HLS_STANDIN_INT_BINOP(*)
HLS_STANDIN_INT_BINOP(/)
#undef HLS_STANDIN_INT_BINOP

#define HLS_STANDIN_CMP(op)                                                                                           \
    template <int W1, int I1, int W2, int I2>                                                                         \
    constexpr bool operator op(const ap_fixed<W1, I1>& a, const ap_fixed<W2, I2>& b)                                  \
    {                                                                                                                 \
        typedef hls_standin::rt<W1, I1, W2, I2> R;                                                                    \
        return hls_standin::regrid(a.pattern(), R::F1, R::sumF) op hls_standin::regrid(b.pattern(), R::F2, R::sumF);  \
    }                                                                                                                 \
    template <int W, int I> constexpr bool operator op(const ap_fixed<W, I>& a, int b) { return a op hls_standin::int_t(b); } \
    template <int W, int I> constexpr bool operator op(int a, const ap_fixed<W, I>& b) { return hls_standin::int_t(a) op b; } \
    template <int W, int I> bool operator op(const ap_fixed<W, I>& a, double b) { static_assert(W < 54, "C2"); return a.to_double() op b; } \
    template <int W, int I> bool operator op(double a, const ap_fixed<W, I>& b) { static_assert(W < 54, "C2"); return a op b.to_double(); }
HLS_STANDIN_CMP(==)
HLS_STANDIN_CMP(!=)
HLS_STANDIN_CMP(<)
HLS_STANDIN_CMP(<=)
HLS_STANDIN_CMP(>)
HLS_STANDIN_CMP(>=)
#undef HLS_STANDIN_CMP

#endif /* HLS_STANDIN_FIXED */
#endif
