// scan.hpp -- the one scan primitive of libsa_hip: a 64-lane inclusive scan and the workgroup scan built on it.
//
// Both layers are generic over the value type T (u32, u64, uint2, a small struct such as big::FlagAgg) and over the
// combine `op(x, y)`, where x covers the elements BEFORE those of y: op only has to be associative, so an ordered combine
// ("the last head seen") scans as well as a sum or a max.  Nothing here launches or synchronises on its own account beyond
// the two barriers that block_scan_excl documents; tile bodies that overlap other work with their barrier call the wave
// layer and keep their own LDS exchange.
#pragma once
#include "common.hpp"
#include <type_traits>

namespace sa {

#if defined(__HIPCC__)
struct ScanSum {   // u32, u64, and uint2 (component-wise: the {active, heads} pairs)
    template <class T> __device__ __forceinline__ T operator()(const T& x, const T& y) const { return x + y; }
    __device__ __forceinline__ uint2 operator()(const uint2& x, const uint2& y) const { return make_uint2(x.x + y.x, x.y + y.y); }
};
struct ScanMax {
    template <class T> __device__ __forceinline__ T operator()(const T& x, const T& y) const { return y > x ? y : x; }
};

// v of the lane `o` below (own v in lanes < o); a T of several 32-bit words moves as one shuffle per word
template <class T>
__device__ __forceinline__ T lane_shift_up(const T& v, int o) {
    if constexpr (std::is_arithmetic<T>::value) {
        return __shfl_up(v, o);
    } else {
        static_assert(sizeof(T) % 4 == 0 && std::is_trivially_copyable<T>::value, "scan values are whole 32-bit words");
        u32 w[sizeof(T) / 4];
        memcpy(w, &v, sizeof(T));
#pragma unroll
        for (u32 k = 0; k < sizeof(T) / 4; ++k) w[k] = __shfl_up(w[k], o);
        T r;
        memcpy(&r, w, sizeof(T));
        return r;
    }
}

// inclusive scan over the 64 lanes of the wave: lane l returns op(v[0], ..., v[l]).  Every lane of the wave must call it.
template <class T, class Op>
__device__ __forceinline__ T wave_scan_incl(T v, Op op) {
    const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const T t = lane_shift_up(v, o);
        if (lane >= o) v = op(t, v);
    }
    return v;
}

// the wave's aggregate op(v[0], ..., v[63]) in every lane: the scan read at lane 63 (a minimum: ~wave_reduce(~key, ScanMax{}))
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
    return __shfl(wave_scan_incl(v, op), WAVE - 1);
}

// exclusive scan over a workgroup of WAVES full waves (thread order): wave scan, lane 63 publishes its wave's total to
// s_w[WAVES], barrier, prefix over the earlier waves, trailing barrier (s_w may be reused at once, e.g. by the next trip of
// a carry loop).  *total, when asked for, is the workgroup's aggregate in every thread.  Every thread must call it.
template <int WAVES, class T, class Op>
__device__ __forceinline__ T block_scan_excl(T v, T identity, Op op, T* s_w, T* total = nullptr) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const T incl = wave_scan_incl(v, op);
    if (lane == WAVE - 1) s_w[wave] = incl;
    T excl = lane_shift_up(incl, 1);
    if (lane == 0) excl = identity;
    __syncthreads();
    T off = identity, tot = identity;
    for (int w = 0; w < WAVES; ++w) {
        const T t = s_w[w];
        if (w < wave) off = op(off, t);
        tot = op(tot, t);
    }
    __syncthreads();
    if (total) *total = tot;
    return op(off, excl);
}
#endif

}  // namespace sa
