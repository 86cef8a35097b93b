// Staging on either side of the generator in the try-on driver (training/tryon.py; the reference's test.py:126-181), on gfx950.
//   pg_tryon_row_extent_u8  first / last non-zero row of every canvas of a batch (the two post-routing bound rules)
//   pg_tryon_inputs         the seven float32 NCHW generator inputs of training.dataset.to_generator_inputs, from uint8 NHWC sources, in one launch
//   pg_tryon_triptych_u8    clothes | person | result, columns x0 : x0 + cw of each, as uint8 RGB rows (test.py:162-181)
//   pg_tryon_panels_u8      the same packing for k source images: source 0 | ... | source k-1 | result (the outfit mode's four panels)
// The results equal torch on the GPU bit for bit: every value is built with the float32 operations torch runs, in its order, and nothing is
// contracted into a fused multiply-add (the pragma below).  torch divides a GPU tensor by the Python scalar 127.5 by multiplying with the rounded
// reciprocal 1.0f / 127.5f (tests/test_tryon_gpu.py pins this over all 256 byte values), so `unit` does the same.
// Memory-bound streams: one lane = 4 consecutive pixels of a row -> 16-byte float4 stores per plane; the uint8 sides are read as dwords.
#include "pg_common.h"
#include "pg_stage.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace {

using namespace pg::stage;       // f32x4, u32x4, unit, byte_of, load_px4, store4 (shared with csrc/train_fetch.hip)

// ----------------------------------------------------------------------------------------------------------- row extents
// One workgroup per canvas: every lane scans 16-byte chunks (a chunk never straddles a row: row_bytes % 16 == 0) and keeps its own first / last
// non-zero row; LDS atomics reduce.  ext[2 i] = first, ext[2 i + 1] = last, -1 / -1 for an empty canvas.
__global__ __launch_bounds__(1024) void row_extent_u8_kernel(const uint8_t* __restrict__ canvases, int h, int row_bytes, int* __restrict__ ext) {
    __shared__ int s_lo, s_hi;
    if (threadIdx.x == 0) { s_lo = 0x7fffffff; s_hi = -1; }
    __syncthreads();
    const int64_t nbytes = (int64_t)h * row_bytes;
    const u32x4* src = reinterpret_cast<const u32x4*>(canvases + (int64_t)blockIdx.x * nbytes);
    const int chunks = (int)(nbytes / 16), per_row = row_bytes / 16;
    int lo = 0x7fffffff, hi = -1;
    for (int i = threadIdx.x; i < chunks; i += blockDim.x) {
        const u32x4 v = __builtin_nontemporal_load(src + i);
        if ((v.x | v.y | v.z | v.w) != 0u) {
            const int r = i / per_row;
            lo = r < lo ? r : lo;
            hi = r > hi ? r : hi;
        }
    }
    if (hi >= 0) {
        atomicMin(&s_lo, lo);
        atomicMax(&s_hi, hi);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ext[2 * blockIdx.x] = s_hi >= 0 ? s_lo : -1;
        ext[2 * blockIdx.x + 1] = s_hi;
    }
}

// ----------------------------------------------------------------------------------------------------------- generator inputs
// Grid: x = big_blocks workgroups over the H x W planes (4 pixels per lane) + the workgroups over the h x w part patches; y = sample.
// The per-sample table (skin medians, label, row extents) is read once per workgroup into LDS.
__global__ __launch_bounds__(256) void inputs_kernel(pg_tryon_io io, int H, int W, int h, int w, int mode, int big_blocks) {
    const int n = blockIdx.y;
    __shared__ float s_skin[3];
    __shared__ float s_label;
    __shared__ int s_lbl, s_lo, s_hi;
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; c++) s_skin[c] = unit(io.skin[3 * n + c]);
        s_lbl = io.label[n];
        s_label = unit((float)s_lbl * 127.5f);                   // lower_label_map = label / 2 * 255 (exact), then unit()
        s_lo = io.extents ? io.extents[2 * n] : -1;
        s_hi = io.extents ? io.extents[2 * n + 1] : -1;
    }
    __syncthreads();
    if ((int)blockIdx.x < big_blocks) {
        const int64_t HW = (int64_t)H * W;
        const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;          // quad index within the sample
        if (q * 4 >= HW) return;
        const int64_t p = q * 4;                                             // first pixel (W % 4 == 0: the quad lies in one row)
        const int y = (int)(p / W);
        const int64_t px = n * HW + p;                                       // pixel index in the batch
        uint32_t im[3], po[3], du[3], dl[3], rm[1];
        load_px4<3>(io.image + px * 3, im);
        load_px4<3>(io.pose + px * 3, po);
        load_px4<3>(io.denorm_upper + px * 3, du);
        load_px4<3>(io.denorm_lower + px * 3, dl);
        load_px4<1>(io.retain_mask + px, rm);

        // retain [N, 6, H, W] = image_t * m - (1 - m), then the three skin planes
        float* rt = io.retain + (int64_t)n * 6 * HW + p;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float m = (float)byte_of(rm, k);
                v[k] = unit((float)byte_of(im, 3 * k + c)) * m - (1.0f - m);
            }
            store4(rt + c * HW, v[0], v[1], v[2], v[3]);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) store4(rt + (3 + c) * HW, s_skin[c], s_skin[c], s_skin[c], s_skin[c]);

        // pose [N, 5, H, W] = pose, label plane, bound plane (the host's row after the mode's post-routing rule)
        float* ps = io.pose_out + (int64_t)n * 5 * HW + p;
#pragma unroll
        for (int c = 0; c < 3; c++)
            store4(ps + c * HW, unit((float)byte_of(po, c)), unit((float)byte_of(po, 3 + c)), unit((float)byte_of(po, 6 + c)),
                   unit((float)byte_of(po, 9 + c)));
        store4(ps + 3 * HW, s_label, s_label, s_label, s_label);
        uint32_t b = io.bound_rows[(int64_t)n * H + y];
        if (mode == PG_TRYON_UPPER) {                                // bound[0:ymax] *= 0, ymax = last row of denorm_upper_img_wo_sleeve
            if (s_hi >= 0 && y < s_hi) b = 0;
        } else if (mode == PG_TRYON_FULL || mode == PG_TRYON_OUTFIT) {       // bound[ymin:] += 255 from the routed lower garment; a dress: bound * 0
            if (s_lbl == 2) b = 0;
            else if (s_lo >= 0 && y >= s_lo) b = (b + 255u) & 0xffu;
        }
        const float bv = unit((float)b);
        store4(ps + 4 * HW, bv, bv, bv, bv);

        // denorm_{upper,lower}_input [N, 3, H, W] and their masks [N, 1, H, W] ("any channel non-zero")
        float* ou = io.denorm_upper_out + (int64_t)n * 3 * HW + p;
        float* ol = io.denorm_lower_out + (int64_t)n * 3 * HW + p;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            store4(ou + c * HW, unit((float)byte_of(du, c)), unit((float)byte_of(du, 3 + c)), unit((float)byte_of(du, 6 + c)),
                   unit((float)byte_of(du, 9 + c)));
            store4(ol + c * HW, unit((float)byte_of(dl, c)), unit((float)byte_of(dl, 3 + c)), unit((float)byte_of(dl, 6 + c)),
                   unit((float)byte_of(dl, 9 + c)));
        }
        float mu[4], ml[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            mu[k] = (byte_of(du, 3 * k) | byte_of(du, 3 * k + 1) | byte_of(du, 3 * k + 2)) ? 1.0f : 0.0f;
            ml[k] = (byte_of(dl, 3 * k) | byte_of(dl, 3 * k + 1) | byte_of(dl, 3 * k + 2)) ? 1.0f : 0.0f;
        }
        store4(io.upper_mask_out + n * HW + p, mu[0], mu[1], mu[2], mu[3]);
        store4(io.lower_mask_out + n * HW + p, ml[0], ml[1], ml[2], ml[3]);
    } else {
        // c [N, 45, h, w] = unit(norm_img [N, h, w, 30]) ++ unit(norm_img_lower [N, h, w, 15])
        const int64_t hw = (int64_t)h * w;
        const int64_t q = (int64_t)(blockIdx.x - big_blocks) * 256 + threadIdx.x;
        if (q * 4 >= hw) return;
        const int64_t p = q * 4;
        uint32_t a[30], l[15];
        load_px4<30>(io.norm_img + (n * hw + p) * 30, a);
        load_px4<15>(io.norm_img_lower + (n * hw + p) * 15, l);
        float* oc = io.c + (int64_t)n * 45 * hw + p;
#pragma unroll
        for (int c = 0; c < 30; c++)
            store4(oc + c * hw, unit((float)byte_of(a, c)), unit((float)byte_of(a, 30 + c)), unit((float)byte_of(a, 60 + c)),
                   unit((float)byte_of(a, 90 + c)));
#pragma unroll
        for (int c = 0; c < 15; c++)
            store4(oc + (30 + c) * hw, unit((float)byte_of(l, c)), unit((float)byte_of(l, 15 + c)), unit((float)byte_of(l, 30 + c)),
                   unit((float)byte_of(l, 45 + c)));
    }
}

// ----------------------------------------------------------------------------------------------------------- triptych
// test.py:162-181 for 4 output pixels per lane.  Result column: clip((x + 1) * 127.5, 0, 255) truncated, NaN -> 0 (NumPy leaves the cast of a NaN
// undefined).  Clothes / person columns: the reference's round trip (u * (1 / 127.5) - 1 + 1) * 127.5 truncated, without a clip: it can land one below u.
__device__ __forceinline__ uint32_t source_byte(uint32_t u) { return (uint32_t)(int)((unit((float)u) + 1.0f) * 127.5f); }
__device__ __forceinline__ uint32_t result_byte(float x) {
    float v = (x + 1.0f) * 127.5f;
    if (v != v) return 0u;
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    return (uint32_t)(int)v;
}

// One kernel body for both packers: K source panels (the triptych: clothes, person; the outfit panels: upper clothes, lower clothes, person), then the
// result.  K is a compile-time constant: the triptych's instance is the kernel it always was.
template <int K> struct PanelSources { const uint8_t* src[K]; };

template <int K>
__global__ __launch_bounds__(256) void panels_u8_kernel(const float* __restrict__ fin, PanelSources<K> srcs, uint8_t* __restrict__ out, int n_rows, int H,
                                                        int W, int x0, int cw) {
    const int qpr = (K + 1) * cw / 4;                                // quads per output row
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)n_rows * qpr) return;
    const int row = (int)(q / qpr), xq = (int)(q - (int64_t)row * qpr) * 4;     // output column of the quad's first pixel
    const int n = row / H, y = row - n * H;
    const int part = xq / cw, x = x0 + xq - part * cw;              // 0 .. K-1 the sources, K the result (cw % 4 == 0: a quad stays in one part)
    uint32_t o[3] = {0u, 0u, 0u};
    if (part < K) {
        uint32_t w[3];
        const uint8_t* s = srcs.src[0];                              // (selected without indexing the kernel argument by a run-time value)
#pragma unroll
        for (int i = 1; i < K; i++) s = part == i ? srcs.src[i] : s;
        load_px4<3>(s + (((int64_t)n * H + y) * W + x) * 3, w);
#pragma unroll
        for (int i = 0; i < 12; i++) o[i >> 2] |= source_byte(byte_of(w, i)) << ((i & 3) * 8);
    } else {
        const int64_t HW = (int64_t)H * W;
        const float* f = fin + (int64_t)n * 3 * HW + (int64_t)y * W + x;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(f + c * HW));
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = 3 * k + c;
                o[i >> 2] |= result_byte(vv[k]) << ((i & 3) * 8);
            }
        }
    }
    uint32_t* d = reinterpret_cast<uint32_t*>(out + ((int64_t)row * (K + 1) * cw + xq) * 3);
#pragma unroll
    for (int i = 0; i < 3; i++) __builtin_nontemporal_store(o[i], d + i);
}

template <int K>
void launch_panels(const float* fin, const unsigned char* const* sources, unsigned char* out, int n, int H, int W, int x0, int cw, int64_t quads,
                   hipStream_t stream) {
    PanelSources<K> srcs;
    for (int i = 0; i < K; i++) srcs.src[i] = sources[i];
    hipLaunchKernelGGL(panels_u8_kernel<K>, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, stream, fin, srcs, out, n * H, H, W, x0, cw);
}

}  // namespace

PG_EXPORT int pg_tryon_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int pg_tryon_row_extent_u8(const unsigned char* canvases, int ncanvases, int h, int w, int channels, int* extents, void* stream) {
    if (!canvases || !extents || ncanvases <= 0 || h <= 0 || w <= 0 || channels <= 0) return PG_ERR_INVALID_ARG;
    if (!pg::aligned16(canvases) || ((int64_t)w * channels) % 16 != 0) return PG_ERR_UNSUPPORTED;
    if ((int64_t)h * w * channels / 16 > 0x7fffffffLL || ncanvases > 0x7fffffff) return PG_ERR_TOO_LARGE;
    hipLaunchKernelGGL(row_extent_u8_kernel, dim3((unsigned)ncanvases), dim3(1024), 0, (hipStream_t)stream, canvases, h, w * channels, extents);
    return pg::launch_status();
}

PG_EXPORT int pg_tryon_inputs(const pg_tryon_io* io, int n, int H, int W, int h, int w, int mode, void* stream) {
    if (!io || n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return PG_ERR_INVALID_ARG;
    if (mode != PG_TRYON_UPPER && mode != PG_TRYON_LOWER && mode != PG_TRYON_FULL && mode != PG_TRYON_OUTFIT) return PG_ERR_INVALID_ARG;
    const void* req[] = {io->image, io->pose, io->retain_mask, io->denorm_upper, io->denorm_lower, io->norm_img, io->norm_img_lower, io->skin, io->label,
                         io->bound_rows, io->c, io->retain, io->pose_out, io->denorm_upper_out, io->denorm_lower_out, io->upper_mask_out, io->lower_mask_out};
    for (const void* p : req)
        if (!p) return PG_ERR_INVALID_ARG;
    if (mode != PG_TRYON_LOWER && !io->extents) return PG_ERR_INVALID_ARG;
    if (W % 4 || w % 4) return PG_ERR_UNSUPPORTED;
    const void* u8[] = {io->image, io->pose, io->retain_mask, io->denorm_upper, io->denorm_lower, io->norm_img, io->norm_img_lower};
    for (const void* p : u8)
        if (reinterpret_cast<uintptr_t>(p) & 3u) return PG_ERR_UNSUPPORTED;
    const void* f32[] = {io->c, io->retain, io->pose_out, io->denorm_upper_out, io->denorm_lower_out, io->upper_mask_out, io->lower_mask_out};
    for (const void* p : f32)
        if (!pg::aligned16(p)) return PG_ERR_UNSUPPORTED;
    if ((int64_t)H * W > 0x3fffffffLL || (int64_t)h * w > 0x3fffffffLL || n > 65535) return PG_ERR_TOO_LARGE;
    const int big = (int)(((int64_t)H * W / 4 + 255) / 256), small = (int)(((int64_t)h * w / 4 + 255) / 256);
    hipLaunchKernelGGL(inputs_kernel, dim3((unsigned)(big + small), (unsigned)n), dim3(256), 0, (hipStream_t)stream, *io, H, W, h, w, mode, big);
    return pg::launch_status();
}

PG_EXPORT int pg_tryon_panels_u8(const float* finetune_img, const unsigned char* const* sources, int k, unsigned char* out, int n, int H, int W, int x0,
                                 int cw, void* stream) {
    if (!finetune_img || !sources || !out || k < 1 || k > PG_TRYON_MAX_PANEL_SOURCES || n <= 0 || H <= 0 || W <= 0 || cw <= 0 || x0 < 0 || x0 + cw > W)
        return PG_ERR_INVALID_ARG;
    uintptr_t bits = reinterpret_cast<uintptr_t>(out);
    for (int i = 0; i < k; i++) {
        if (!sources[i]) return PG_ERR_INVALID_ARG;
        bits |= reinterpret_cast<uintptr_t>(sources[i]);
    }
    if (x0 % 4 || cw % 4 || W % 4 || !pg::aligned16(finetune_img) || (bits & 3u)) return PG_ERR_UNSUPPORTED;
    const int64_t quads = (int64_t)n * H * ((k + 1) * cw / 4);
    if (quads / 256 + 1 > 0x7fffffffLL || (int64_t)H * W > 0x3fffffffLL || (int64_t)n * H > 0x7fffffffLL) return PG_ERR_TOO_LARGE;
    if (k == 1) launch_panels<1>(finetune_img, sources, out, n, H, W, x0, cw, quads, (hipStream_t)stream);
    else if (k == 2) launch_panels<2>(finetune_img, sources, out, n, H, W, x0, cw, quads, (hipStream_t)stream);
    else launch_panels<3>(finetune_img, sources, out, n, H, W, x0, cw, quads, (hipStream_t)stream);
    return pg::launch_status();
}

PG_EXPORT int pg_tryon_triptych_u8(const float* finetune_img, const unsigned char* clothes, const unsigned char* image, unsigned char* out, int n, int H,
                                   int W, int x0, int cw, void* stream) {
    const unsigned char* sources[2] = {clothes, image};
    return pg_tryon_panels_u8(finetune_img, sources, 2, out, n, H, W, x0, cw, stream);
}
