/*
 * hls_vector.h -- stand-in for the Vitis HLS header (own text; see ap_fixed.h).  hls::vector<T, N> is N elements of T
 * with element-wise + - * / and scalar (x) vector forms.  Every operator yields T per element: in the fixed form each
 * product or quotient is stored to T before the next operation (rule R7 of oracle/q_oracle.c).
 */
#ifndef HLS_STANDIN_HLS_VECTOR_H
#define HLS_STANDIN_HLS_VECTOR_H

#include <array> /* the reference relies on the Vitis header bringing std::array in */
#include <cstddef>

namespace hls {
template <typename T, size_t N>
struct vector {
    T data[N];
    vector() = default;
    vector(const T& x) { for (size_t i = 0; i < N; i++) data[i] = x; }
    T& operator[](size_t i) { return data[i]; }
    const T& operator[](size_t i) const { return data[i]; }
    static constexpr size_t size() { return N; }

#define HLS_STANDIN_VEC_OP(op)                                                                                        \
    vector& operator op##=(const vector& o) { for (size_t i = 0; i < N; i++) data[i] = T(data[i] op o.data[i]); return *this; } \
    vector& operator op##=(const T& o) { for (size_t i = 0; i < N; i++) data[i] = T(data[i] op o); return *this; }      \
    friend vector operator op(const vector& a, const vector& b) { vector r; for (size_t i = 0; i < N; i++) r.data[i] = T(a.data[i] op b.data[i]); return r; } \
    friend vector operator op(const vector& a, const T& b) { vector r; for (size_t i = 0; i < N; i++) r.data[i] = T(a.data[i] op b); return r; } \
    friend vector operator op(const T& a, const vector& b) { vector r; for (size_t i = 0; i < N; i++) r.data[i] = T(a op b.data[i]); return r; }
    HLS_STANDIN_VEC_OP(+)
    HLS_STANDIN_VEC_OP(-)
    HLS_STANDIN_VEC_OP(*)
    HLS_STANDIN_VEC_OP(/)
#undef HLS_STANDIN_VEC_OP
};
}  // namespace hls
#endif
