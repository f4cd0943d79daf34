// gfx950 read-out kernels of the witness engine (export.hpp): cells of a stream
// range or a strided view, written dense in canonical or Montgomery form, or
// dequantized to f64. One cell per lane (two 16 B loads, two 16 B stores),
// grid-stride over a capped grid, 64-bit indices: a 4096^2 stream holds more
// than 2^31 cells.
#include <hip/hip_runtime.h>

#include "export.hpp"

namespace svdw {

static constexpr unsigned kExportThreads = 256;
static constexpr unsigned kExportMaxBlocks = 8192;   // 256 CUs x 8 blocks x 4 rounds

// index of cell k in the source stream
template <bool VIEW>
__device__ __forceinline__ int64_t export_index(const ExportSrc& s, uint64_t k) {
    if (!VIEW) return (int64_t)(s.off + k);
    uint64_t i, j;
    k += s.k0;
    if (s.k0 + s.n <= 0xffffffffull) {                   // (uniform) the short division
        const uint32_t kk = (uint32_t)k;
        i = kk / s.cols;
        j = kk - (uint32_t)i * s.cols;
    } else {
        i = k / s.cols;
        j = k - i * s.cols;
    }
    return (int64_t)s.off + (int64_t)i * s.rs + (int64_t)j * s.cs;
}

template <int FORM, bool VIEW>
__global__ __launch_bounds__(kExportThreads) void k_export(const ExportSrc s, Fr* __restrict__ dst, uint64_t pad) {
    const uint64_t total = s.n + pad, step = (uint64_t)gridDim.x * kExportThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kExportThreads + threadIdx.x; k < total; k += step) {
        Fr x = fr_zero();
        if (k < s.n) {
            x = ld_fr(s.src + export_index<VIEW>(s, k));
            if (FORM == kFormMontgomery) x = fr_to_mont(x);
        }
        st_fr(dst + k, x);
    }
}

template <bool VIEW>
__global__ __launch_bounds__(kExportThreads) void k_dequantize(const ExportSrc s, uint32_t P, double* __restrict__ dst) {
    const uint64_t step = (uint64_t)gridDim.x * kExportThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kExportThreads + threadIdx.x; k < s.n; k += step)
        dst[k] = dequantize_fr(ld_fr(s.src + export_index<VIEW>(s, k)), P);
}

static unsigned export_blocks(uint64_t total) {
    const uint64_t b = (total + kExportThreads - 1) / kExportThreads;
    return (unsigned)(b < kExportMaxBlocks ? b : kExportMaxBlocks);
}

hipError_t launch_export(const ExportSrc& s, int form, Fr* dst, uint64_t pad, hipStream_t st) {
    const uint64_t total = s.n + pad;
    if (!total) return hipSuccess;
    if (!dst || (s.n && !s.src) || (form != kFormCanonical && form != kFormMontgomery)) return hipErrorInvalidValue;
    const dim3 g(export_blocks(total)), b(kExportThreads);
    const bool view = s.cols != 0;
    if (form == kFormMontgomery) {
        if (view) hipLaunchKernelGGL((k_export<kFormMontgomery, true>), g, b, 0, st, s, dst, pad);
        else hipLaunchKernelGGL((k_export<kFormMontgomery, false>), g, b, 0, st, s, dst, pad);
    } else {
        if (view) hipLaunchKernelGGL((k_export<kFormCanonical, true>), g, b, 0, st, s, dst, pad);
        else hipLaunchKernelGGL((k_export<kFormCanonical, false>), g, b, 0, st, s, dst, pad);
    }
    return hipGetLastError();
}

hipError_t launch_dequantize(const ExportSrc& s, uint32_t P, double* dst, hipStream_t st) {
    if (!s.n) return hipSuccess;
    if (!dst || !s.src || P < 1 || P > 63) return hipErrorInvalidValue;
    const dim3 g(export_blocks(s.n)), b(kExportThreads);
    if (s.cols) hipLaunchKernelGGL((k_dequantize<true>), g, b, 0, st, s, P, dst);
    else hipLaunchKernelGGL((k_dequantize<false>), g, b, 0, st, s, P, dst);
    return hipGetLastError();
}

}  // namespace svdw
