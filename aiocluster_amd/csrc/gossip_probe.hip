// gossip_probe.hip -- the measurement kernels of libgossip_sim.so: gs_stream_copy / _read / _write and gs_mark.

#include "gossip_common.h"

namespace {

// ------------------------------------------------------------------ measurement kernels
// Streaming copy: the measured HBM ceiling bench.py reports beside the 8 TB/s peak.  And read-only / write-only
// streams at 4, 8 or 16 B per lane whose known byte counts calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE.
// measurement kernels (gs_stream_copy / _read / _write).  The copy: each wave moves contiguous 16 KiB chunks
// (64 lanes x 16 B x 16 loads in flight per lane, non-temporal loads and stores), chunks dealt grid-stride
// over 65,536 workgroups -- the fastest copy shape of tools/membench8.hip on the box (5.99 TB/s vs 5.30 for
// round 3's grid-stride 8-deep copy, r4b)
__global__ __launch_bounds__(256) void k_copy16(v4u_t *__restrict__ dst, const v4u_t *__restrict__ src, uint64_t n16) {
    const uint64_t waves = (uint64_t)gridDim.x * 4u, wid = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t chunks = n16 / 1024u;
    for (uint64_t c = wid; c < chunks; c += waves) {
        const uint64_t b = c * 1024u + lane;
        v4u_t v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = __builtin_nontemporal_load(src + b + u * 64);
#pragma unroll
        for (int u = 0; u < 16; u++) __builtin_nontemporal_store(v[u], dst + b + u * 64);
    }
    // the tail (< 16 KiB): grid-stride
    for (uint64_t i = chunks * 1024u + (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n16; i += waves * 64u) dst[i] = src[i];
}
template <typename V>
__global__ __launch_bounds__(256) void k_write(V *__restrict__ dst, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    V v;
    memset(&v, 0x5A, sizeof v);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) dst[i] = v;
}
__device__ __forceinline__ uint32_t fold(uint32_t v) { return v; }
__device__ __forceinline__ uint32_t fold(uint2 v) { return v.x ^ v.y; }
__device__ __forceinline__ uint32_t fold(uint4 v) { return v.x ^ v.y; }
template <typename V>
__global__ __launch_bounds__(256) void k_read(const V *__restrict__ src, uint64_t n, unsigned long long *sink) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    uint32_t acc = 0;
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        const V a = src[i], b = src[i + stride], c = src[i + 2 * stride], e = src[i + 3 * stride];
        acc ^= fold(a) ^ fold(b) ^ fold(c) ^ fold(e);
    }
    for (; i < n; i += stride) acc ^= fold(src[i]);
    if (acc == 0x9E3779B9u) atomicAdd(sink, 1ull);  // keeps the loads; practically never taken
}

// gs_mark: empty one-wave dispatches whose names bracket a region of a kernel trace (bench.py's timed rounds), so
// tools/pmc_summary.py averages exactly the dispatches between them
__global__ __launch_bounds__(WAVE) void k_mark_begin() {}
__global__ __launch_bounds__(WAVE) void k_mark_end() {}

}  // namespace

extern "C" {

int gs_stream_copy(void *dst, const void *src, uint64_t bytes, void *stream) {
    if (!dst || !src || (bytes & 15u) || ((uintptr_t)dst & 15u) || ((uintptr_t)src & 15u)) return GS_E_INVALID;
    k_copy16<<<65536, 256, 0, (hipStream_t)stream>>>((v4u_t *)dst, (const v4u_t *)src, bytes / 16);
    return hipGetLastError() == hipSuccess ? GS_OK : GS_E_HIP;
}

int gs_stream_write(void *dst, uint64_t bytes, uint32_t width, void *stream) {
    if (!dst || (width != 4 && width != 8 && width != 16) || (bytes % width) || ((uintptr_t)dst & 15u))
        return GS_E_INVALID;
    if (width == 4)
        k_write<uint32_t><<<32768, 256, 0, (hipStream_t)stream>>>((uint32_t *)dst, bytes / 4);
    else if (width == 8)
        k_write<uint2><<<32768, 256, 0, (hipStream_t)stream>>>((uint2 *)dst, bytes / 8);
    else
        k_write<uint4><<<32768, 256, 0, (hipStream_t)stream>>>((uint4 *)dst, bytes / 16);
    return hipGetLastError() == hipSuccess ? GS_OK : GS_E_HIP;
}

int gs_stream_read(const void *src, uint64_t bytes, uint32_t width, uint64_t *sink, void *stream) {
    if (!src || !sink || (width != 4 && width != 8 && width != 16) || (bytes % width) || ((uintptr_t)src & 15u))
        return GS_E_INVALID;
    if (width == 4)
        k_read<uint32_t><<<32768, 256, 0, (hipStream_t)stream>>>((const uint32_t *)src, bytes / 4,
                                                                 (unsigned long long *)sink);
    else if (width == 8)
        k_read<uint2><<<32768, 256, 0, (hipStream_t)stream>>>((const uint2 *)src, bytes / 8,
                                                              (unsigned long long *)sink);
    else
        k_read<uint4><<<32768, 256, 0, (hipStream_t)stream>>>((const uint4 *)src, bytes / 16,
                                                              (unsigned long long *)sink);
    return hipGetLastError() == hipSuccess ? GS_OK : GS_E_HIP;
}

int gs_mark(uint32_t which, void *stream) {
    if (which > 1) return GS_E_INVALID;
    if (which == 0)
        k_mark_begin<<<1, WAVE, 0, (hipStream_t)stream>>>();
    else
        k_mark_end<<<1, WAVE, 0, (hipStream_t)stream>>>();
    return hipGetLastError() == hipSuccess ? GS_OK : GS_E_HIP;
}

}  // extern "C"
