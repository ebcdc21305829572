/*
 * check.cc -- stand-alone self-check of the FIXED form of the stand-in headers (make -C oracle check-standin; with SANITIZE=1 under
 * UBSan + ASan, which is how tests/test_reference_pin_cpu.py runs it: the check guards the stand-in's own shifts and overflows).
 * Every rule is compared with a plain integer formula on 16-bit patterns, exhaustively over one operand and sampled over the other,
 * for both formats the reference uses: ap_fixed<16,6> and ap_fixed<16,3>.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ap_fixed.h"
#include "hls_math.h"
#include "hls_stream.h"
#include "hls_vector.h"

static long g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        g_checks++;                                                                                      \
        if (!(cond)) {                                                                                   \
            if (g_failures++ < 20) std::fprintf(stderr, "%s:%d: %s  (a=%d b=%d)\n", __FILE__, __LINE__, #cond, (int)pa, (int)pb); \
        }                                                                                                \
    } while (0)

static int16_t wrap16(int64_t x) { return (int16_t)(uint16_t)(uint64_t)x; }
static int64_t floor_shift(int64_t x, int k) { return x >= 0 ? x / ((int64_t)1 << k) : -((-x + ((int64_t)1 << k) - 1) / ((int64_t)1 << k)); }
static int64_t trunc_div(int64_t a, int64_t b) { return a / b; } /* C++ integer division truncates toward zero */
static uint64_t isqrt_ref(uint64_t x)
{
    uint64_t r = 0;
    for (uint64_t bit = (uint64_t)1 << 31; bit; bit >>= 1)
        if ((r + bit) * (r + bit) <= x) r += bit;
    return r;
}

template <int I>
static void check_format(const std::vector<int>& samples)
{
    typedef ap_fixed<16, I> T;
    constexpr int F = 16 - I;
    static_assert(T::width == 16 && T::iwidth == I && sizeof(T) == 2, "a 16-bit ap_fixed is one int16_t");
    for (int a = -32768; a < 32768; a++) {
        const int16_t pa = (int16_t)a;
        int16_t pb = 0;
        const T x = T::from_pattern(pa);
        CHECK(x.v == pa);
        /* conversions */
        CHECK(x.to_double() == (double)pa / (double)(1 << F));
        CHECK(x.to_float() == (float)((double)pa / (double)(1 << F)));
        CHECK(x.to_int() == pa / (1 << F));                                          /* toward zero */
        CHECK(T(x.to_double()).v == pa);
        CHECK(T(x.to_double() + 0.3 / (1 << F)).v == pa);                       /* floor, not round */
        CHECK(T(x.to_double() - 0.3 / (1 << F)).v == wrap16((int64_t)pa - 1));  /* floor toward -inf, wraps below the minimum */
        CHECK(T(x.to_double() + (double)(1 << I)).v == pa);                     /* one full turn: AP_WRAP */
        CHECK(T((float)x.to_double()).v == pa);
        CHECK(T(a).v == wrap16((int64_t)a * (1 << F)));                          /* int -> ap_fixed wraps */
        /* unary minus, abs, signbit, comparisons with literals */
        CHECK((-x).pattern() == -(int64_t)pa && T(-x).v == wrap16(-(int64_t)pa));
        CHECK(hls::abs(x).v == wrap16(pa < 0 ? -(int64_t)pa : pa));
        CHECK(hls::signbit(x) == (pa < 0));
        CHECK((x == 0.0) == (pa == 0) && (x == 0) == (pa == 0) && (x < 0) == (pa < 0) && (x > 0) == (pa > 0));
        CHECK((x >= 1) == (pa >= (1 << F)) && (1 <= x) == (pa >= (1 << F)));
        /* R3 / R4 / R5 */
        CHECK(hls::sqrt(x).v == (pa <= 0 ? 0 : wrap16((int64_t)isqrt_ref((uint64_t)pa << F))));
        CHECK(hls::recip(x).v == (pa <= 0 ? 0 : wrap16(((int64_t)1 << (2 * F)) / pa)));
        {
            double e = std::floor(std::exp((double)pa / (1 << F)) * (1 << F));
            CHECK(hls::exp(x).v == (e >= 9.0e18 ? 0 : wrap16((int64_t)e)));
            CHECK(hls::log(x).v == (pa <= 0 ? 0 : wrap16((int64_t)std::floor(std::log((double)pa / (1 << F)) * (1 << F)))));
        }
        /* division by an int: quotient with F + 32 fractional bits, truncated toward zero, floored on store */
        for (int n : samples) {
            pb = (int16_t)n;
            int64_t q = n == 0 ? 0 : trunc_div((int64_t)pa * ((int64_t)1 << 32), n);
            CHECK((x / n).pattern() == q);
            CHECK(T(x / n).v == wrap16(floor_shift(q, 32)));
            CHECK((x * n).pattern() == (int64_t)pa * n && (x + n).pattern() == (int64_t)pa + (int64_t)n * (1 << F));
            CHECK((n - x).pattern() == (int64_t)n * (1 << F) - pa);
        }
        for (int b : samples) {
            pb = (int16_t)b;
            const T y = T::from_pattern(pb);
            /* exact wide results, then the store */
            CHECK((x + y).pattern() == (int64_t)pa + pb && T(x + y).v == wrap16((int64_t)pa + pb));
            CHECK((x - y).pattern() == (int64_t)pa - pb && T(x - y).v == wrap16((int64_t)pa - pb));
            CHECK((x * y).pattern() == (int64_t)pa * pb && T(x * y).v == wrap16(floor_shift((int64_t)pa * pb, F)));
            CHECK(decltype(x * y)::width == 32 && decltype(x * y)::iwidth == 2 * I);
            CHECK(decltype(x + y)::width == 17 && decltype(x + y)::iwidth == I + 1);
            CHECK(decltype(x / y)::width - decltype(x / y)::iwidth == F + I);
            int64_t q = pb == 0 ? 0 : trunc_div((int64_t)pa * 65536, pb); /* F + I = 16 fractional bits */
            CHECK((x / y).pattern() == q && T(x / y).v == wrap16(floor_shift(q, I)));
            /* an expression is exact until it is stored: x * y + y * y floors once, not twice */
            CHECK(T(x * y + y * y).v == wrap16(floor_shift((int64_t)pa * pb + (int64_t)pb * pb, F)));
            CHECK(T((x - y) / y * y + x).v == wrap16(floor_shift((pb == 0 ? 0 : trunc_div(((int64_t)pa - pb) * 65536, pb)) * pb + (int64_t)pa * ((int64_t)1 << (F + I)), F + I)));
            /* compound assignment: wide, then stored */
            T r = x; r += y * y;  CHECK(r.v == wrap16((int64_t)pa + floor_shift((int64_t)pb * pb, F)));
            r = x; r -= y;        CHECK(r.v == wrap16((int64_t)pa - pb));
            r = x; r *= y;        CHECK(r.v == wrap16(floor_shift((int64_t)pa * pb, F)));
            r = x; r /= y;        CHECK(r.v == wrap16(floor_shift(q, I)));
            /* comparisons */
            CHECK((x < y) == (pa < pb) && (x <= y) == (pa <= pb) && (x == y) == (pa == pb) && (x != y) == (pa != pb) && (x > y) == (pa > pb) && (x >= y) == (pa >= pb));
            /* the other format: fractions are aligned to the finer grid */
            typedef ap_fixed<16, 9 - I> U; /* I = 6 -> <16,3>, I = 3 -> <16,6> */
            constexpr int FU = 16 - (9 - I), FM = F > FU ? F : FU;
            const U z = U::from_pattern(pb);
            CHECK((x + z).pattern() == (int64_t)pa * (1 << (FM - F)) + (int64_t)pb * (1 << (FM - FU)));
            CHECK(T(z).v == wrap16(FU > F ? floor_shift(pb, FU - F) : (int64_t)pb * (1 << (F - FU))));
            /* hls::vector yields T per element (each product stored before the sum) */
            hls::vector<T, 2> v, w;
            v[0] = x; v[1] = y; w[0] = y; w[1] = y;
            hls::vector<T, 2> p = v * w, s = v * w + w, d = v / w, k = x * w;
            CHECK(p[0].v == wrap16(floor_shift((int64_t)pa * pb, F)) && p[1].v == wrap16(floor_shift((int64_t)pb * pb, F)));
            CHECK(s[0].v == wrap16((int64_t)p[0].v + pb) && d[0].v == wrap16(floor_shift(q, I)) && k[1].v == p[0].v);
        }
    }
}

int main()
{
    std::vector<int> samples = {0, 1, -1, 2, -2, 3, 7, -7, 1023, 1024, 1025, -1024, 8191, 8192, -8192, 16384, 32767, -32767, -32768, 204, -205};
    uint32_t s = 12345u;
    for (int i = 0; i < 43; i++) {
        s = s * 1664525u + 1013904223u;
        samples.push_back((int)(int16_t)(s >> 16));
    }
    check_format<6>(samples);
    check_format<3>(samples);
    {
        int16_t pa = 0, pb = 0;
        /* the literals the reference mixes in */
        CHECK((ap_fixed<16, 6>(0.2)).v == 204 && (ap_fixed<16, 6>(-0.2)).v == -205 && (ap_fixed<16, 6>(0.0)).v == 0);
        CHECK((ap_fixed<16, 6>(1.0 / (1 << 10))).v == 1 && (ap_fixed<16, 3>(1.0 / (1 << 13))).v == 1);
        CHECK((ap_fixed<16, 3>(4.0)).v == -32768 && (ap_fixed<16, 6>(40)).v == wrap16(40 * 1024));
        /* (1 + eps) * h with int 1: ap_fixed<32,32> + ap_fixed<16,6> */
        ap_fixed<16, 6> eps = ap_fixed<16, 6>::from_pattern(3), h = ap_fixed<16, 6>::from_pattern(-700);
        CHECK((ap_fixed<16, 6>((1 + eps) * h)).v == wrap16(floor_shift((int64_t)(1024 + 3) * -700, 10)));
        /* streams are FIFOs */
        hls::stream<int> st("check");
        st << 1; st << 2; st.write(3);
        int u = 0, v = 0;
        st >> u; st >> v;
        CHECK(u == 1 && v == 2 && st.read() == 3 && st.empty());
    }
    std::printf("hls_standin check: %ld checks, %ld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
