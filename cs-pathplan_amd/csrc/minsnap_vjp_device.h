// minsnap_vjp_device.h -- device helpers of the open-chain solve's reverse-mode kernel (minsnap_vjp.hip): record loads,
// d_bar = M(T)^-T p_bar, powers of T and the in-wave sum.  All forced inline, so a kernel that includes them compiles to
// what it would with the text in its own file.
#pragma once
#include "minsnap_device.h"

namespace csp {
namespace vjpk {

template <typename IO, typename R>
__device__ __forceinline__ void vload3(const IO *p, R (&v)[3]) { v[0] = R(p[0]); v[1] = R(p[1]); v[2] = R(p[2]); }

// One segment's p_bar record [3][2O] as 16-byte (f64) or 8-byte (f32) vector loads: record bases are multiples of
// 2O*sizeof(IO) bytes from a 16-byte (f64) / 8-byte (f32) aligned array (checked by the C-ABI).
template <int O, typename IO, typename R>
__device__ __forceinline__ void load_rec(const IO *src, R (&q)[3][2 * O]) {
    typedef IO vec2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
#pragma unroll
        for (int i = 0; i < 2 * O; i += 2) {
            const vec2 v = *reinterpret_cast<const vec2 *>(src + ax * 2 * O + i);
            q[ax][i] = R(v.x);
            q[ax][i + 1] = R(v.y);
        }
}

// d_bar[a] = T^deriv_a sum_i G[i][a] T^-pow_i p_bar[i]  (= M(T)^-T p_bar), for the slots a in [A0, A1)
template <int O, int A0, int A1, typename R>
__device__ __forceinline__ void dbar_axis(const R (&pb)[2 * O], const R (&tp)[O], const R (&ip)[2 * O], R (&db)[2 * O]) {
    constexpr int M = 2 * O;
    R ph[M];
#pragma unroll
    for (int i = 0; i < M; ++i) ph[i] = pb[i] * ip[M - 1 - i];
#pragma unroll
    for (int a = A0; a < A1; ++a) {
        R acc = R(0);
#pragma unroll
        for (int i = 0; i < M; ++i) {
            constexpr double zero = 0.0;
            if (Tab<O>::G(i, a) != zero) acc = fma_<R>(R(Tab<O>::G(i, a)), ph[i], acc);
        }
        db[a] = acc * tp[a % O];
    }
}

template <int O, typename R> __device__ __forceinline__ void powers(R T, R (&tp)[O], R (&ip)[2 * O]) {
    tp[0] = R(1);
#pragma unroll
    for (int e = 1; e < O; ++e) tp[e] = tp[e - 1] * T;
    ip[0] = R(1);
    ip[1] = fast_rcp(T);
#pragma unroll
    for (int e = 2; e < 2 * O; ++e) ip[e] = ip[e - 1] * ip[1];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace vjpk
}  // namespace csp
