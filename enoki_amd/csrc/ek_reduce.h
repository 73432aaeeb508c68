// The reducer semantics and the workgroup fold shared by the horizontal reductions (reduce.hip: one value per array) and
// the block reductions (block_reduce.hip: one value per block of consecutive entries).
#pragma once

#include "ek_map.h"

#include <limits>

namespace ek {

template <int Op, typename T> struct Reducer {
    static __device__ __host__ __forceinline__ T identity() {
        if constexpr (Op == EK_HSUM) return T(0);
        else if constexpr (Op == EK_HPROD) return T(1);
        else if constexpr (std::is_floating_point_v<T>) return std::numeric_limits<T>::quiet_NaN();   // minNum / maxNum: see combine()
        else if constexpr (Op == EK_HMIN) return std::numeric_limits<T>::max();
        else return std::numeric_limits<T>::lowest();
    }
    static __device__ __forceinline__ T combine(T acc, T v) {
        using U = wrap_t<T>;
        if constexpr (Op == EK_HSUM) return (T) ((U) acc + (U) v);
        else if constexpr (Op == EK_HPROD) return (T) ((U) acc * (U) v);
        else if constexpr (std::is_floating_point_v<T>) {
            // Floating point hmin / hmax are IEEE minNum / maxNum reductions (v_min_f32 / v_max_f32): NaN entries are
            // ignored unless every entry is NaN, and -0 < +0 -- well defined and independent of the reduction order.
            // The reference's AVX path is NOT: MINPS returns its second operand on unordered or equal compares, so
            // whether a NaN (or which zero) survives depends on its position modulo the packet width
            // (dynamic.h:669-702); on NaN-free data without mixed zeros both agree bit for bit.
            if constexpr (sizeof(T) == 4) return Op == EK_HMIN ? __builtin_fminf(acc, v) : __builtin_fmaxf(acc, v);
            else return Op == EK_HMIN ? __builtin_fmin(acc, v) : __builtin_fmax(acc, v);
        }
        else if constexpr (Op == EK_HMIN) return v < acc ? v : acc;
        else return v > acc ? v : acc;
    }
};

template <typename T> __device__ __forceinline__ T shfl_down(T v, int delta) {
    if constexpr (sizeof(T) == 8) {
        uint64_t u;
        __builtin_memcpy(&u, &v, 8);
        uint32_t lo = (uint32_t) u, hi = (uint32_t) (u >> 32);
        lo = __shfl_down(lo, delta, 64);
        hi = __shfl_down(hi, delta, 64);
        u = ((uint64_t) hi << 32) | lo;
        __builtin_memcpy(&v, &u, 8);
        return v;
    } else {
        return __shfl_down(v, delta, 64);
    }
}

// 256 threads -> one value in thread 0
template <typename R, typename T> __device__ __forceinline__ T block_reduce(T v) {
    __shared__ T wave_part[4];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v = R::combine(v, shfl_down(v, d));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        v = R::combine(R::combine(wave_part[0], wave_part[1]), R::combine(wave_part[2], wave_part[3]));
    return v;
}

} // namespace ek
