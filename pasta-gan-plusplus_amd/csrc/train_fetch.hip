// The data fetch of the training loop (training/train_fetch.py; the reference's training_loop_fullbody.py:549-601 and the tail of its loader,
// training/dataset.py:1146-1170 and :1223-1241), on gfx950.
//   pg_train_fetch   the nine float32 NCHW tensors of a TrainingStep round from the uint8 NHWC loader planes and the routing's outputs, in one launch
// The erase of the lower-garment patches and the random inpainting mask are applied while reading: no intermediate tensor exists.  Results equal
// torch on the GPU bit for bit, as in csrc/tryon.hip: float32 operations in torch's order, `u / 127.5` as `u * (1.0f / 127.5f)`, no contraction.
// Memory-bound stream: one lane = 4 consecutive pixels of a row -> 16-byte non-temporal stores per plane; the uint8 sides are read as dwords.
#include "pg_common.h"
#include "pg_stage.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace {

using namespace pg::stage;

// Grid: x = big_blocks workgroups over the H x W planes (4 pixels per lane) + the workgroups over the h x w part patches; y = sample.
// The per-sample table (skin medians, label, erase decision, row extent of the routed lower mask) is read once per workgroup into LDS.
__global__ __launch_bounds__(256) void train_fetch_kernel(pg_train_io io, int H, int W, int h, int w, int big_blocks) {
    const int n = blockIdx.y;
    __shared__ float s_skin[3];
    __shared__ float s_label;
    __shared__ int s_kind, s_rows, s_ty, s_by, s_rm;
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; c++) s_skin[c] = unit(io.skin[3 * n + c]);
        s_label = unit((float)io.label[n] * 127.5f);             // lower_label_map = label / 2 * 255 (exact), then unit()
        const int ty = io.extents[2 * n];                        // first row of the routed lower mask of part 0; -1: empty, the record is ignored
        const int kind = ty >= 0 ? io.erase[4 * n] : PG_ERASE_NONE;
        s_kind = kind;
        s_rows = (kind == PG_ERASE_DROP_PART0 && io.erase[4 * n + 1]) ? io.erase[4 * n + 2] : 0;
        s_ty = ty;
        int by = ty + 1 + (int)floorf(io.band_u[n] * (float)(h - ty));   // uniform on ty + 1 ... h for u in [0, 1)
        s_by = by > h ? h : by;
        s_rm = io.random_mask != nullptr && io.erase[4 * n + 3] != 0;
    }
    __syncthreads();
    if ((int)blockIdx.x < big_blocks) {
        const int64_t HW = (int64_t)H * W;
        const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;          // quad index within the sample
        if (q * 4 >= HW) return;
        const int64_t p = q * 4;                                             // first pixel (W % 4 == 0: the quad lies in one row)
        const int y = (int)(p / W);
        const int64_t px = n * HW + p;                                       // pixel index in the batch
        uint32_t im[3], po[3], du[3], dl[3], rm[1], gt[1], rk[1] = {0u};
        load_px4<3>(io.image + px * 3, im);
        load_px4<3>(io.pose + px * 3, po);
        load_px4<3>(io.denorm_upper + px * 3, du);
        load_px4<3>(io.denorm_lower + px * 3, dl);
        load_px4<1>(io.retain_mask + px, rm);
        load_px4<1>(io.gt_parsing + px, gt);
        if (s_rm) load_px4<1>(io.random_mask + px, rk);

        // real_img [N, 3, H, W] and retain [N, 6, H, W] = real * m - (1 - m), then the three skin planes
        float* re = io.real_img + (int64_t)n * 3 * HW + p;
        float* rt = io.retain + (int64_t)n * 6 * HW + p;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float r[4], v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t mb = byte_of(rm, k);                          // `1 - mask` is uint8 arithmetic in the reference (the mask is 0 / 1)
                r[k] = unit((float)byte_of(im, 3 * k + c));
                v[k] = (float)mb * r[k] - (float)((1u - mb) & 0xffu);
            }
            store4(re + c * HW, r[0], r[1], r[2], r[3]);
            store4(rt + c * HW, v[0], v[1], v[2], v[3]);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) store4(rt + (3 + c) * HW, s_skin[c], s_skin[c], s_skin[c], s_skin[c]);

        // pose [N, 5, H, W] = pose, label plane, the for-train bound plane from its row bytes
        float* ps = io.pose_out + (int64_t)n * 5 * HW + p;
#pragma unroll
        for (int c = 0; c < 3; c++)
            store4(ps + c * HW, unit((float)byte_of(po, c)), unit((float)byte_of(po, 3 + c)), unit((float)byte_of(po, 6 + c)),
                   unit((float)byte_of(po, 9 + c)));
        store4(ps + 3 * HW, s_label, s_label, s_label, s_label);
        const float bv = unit((float)io.bound_rows[(int64_t)n * H + y]);
        store4(ps + 4 * HW, bv, bv, bv, bv);

        // gt_parsing [N, 1, H, W]: the label byte as float
        store4(io.gt_parsing_out + n * HW + p, (float)byte_of(gt, 0), (float)byte_of(gt, 1), (float)byte_of(gt, 2), (float)byte_of(gt, 3));

        // denorm_{upper,lower}_input [N, 3, H, W] = canvas * (1 - (random_mask > 0)), and their masks [N, 1, H, W] (channel sum > 0)
        float* ou = io.denorm_upper_out + (int64_t)n * 3 * HW + p;
        float* ol = io.denorm_lower_out + (int64_t)n * 3 * HW + p;
        uint32_t keep[4];
#pragma unroll
        for (int k = 0; k < 4; k++) keep[k] = byte_of(rk, k) ? 0u : 0xffu;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            store4(ou + c * HW, unit((float)(byte_of(du, c) & keep[0])), unit((float)(byte_of(du, 3 + c) & keep[1])),
                   unit((float)(byte_of(du, 6 + c) & keep[2])), unit((float)(byte_of(du, 9 + c) & keep[3])));
            store4(ol + c * HW, unit((float)(byte_of(dl, c) & keep[0])), unit((float)(byte_of(dl, 3 + c) & keep[1])),
                   unit((float)(byte_of(dl, 6 + c) & keep[2])), unit((float)(byte_of(dl, 9 + c) & keep[3])));
        }
        float mu[4], ml[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            mu[k] = ((byte_of(du, 3 * k) | byte_of(du, 3 * k + 1) | byte_of(du, 3 * k + 2)) & keep[k]) ? 1.0f : 0.0f;
            ml[k] = ((byte_of(dl, 3 * k) | byte_of(dl, 3 * k + 1) | byte_of(dl, 3 * k + 2)) & keep[k]) ? 1.0f : 0.0f;
        }
        store4(io.upper_mask_out + n * HW + p, mu[0], mu[1], mu[2], mu[3]);
        store4(io.lower_mask_out + n * HW + p, ml[0], ml[1], ml[2], ml[3]);
    } else {
        // style_input [N, 45, h, w] = unit(norm_img [N, h, w, 30]) ++ unit(erased norm_img_lower [N, h, w, 15])
        const int64_t hw = (int64_t)h * w;
        const int64_t q = (int64_t)(blockIdx.x - big_blocks) * 256 + threadIdx.x;
        if (q * 4 >= hw) return;
        const int64_t p = q * 4;
        const int y = (int)(p / w);                                          // (w % 4 == 0: the quad lies in one row)
        uint32_t a[30], l[15];
        load_px4<30>(io.norm_img + (n * hw + p) * 30, a);
        load_px4<15>(io.norm_img_lower + (n * hw + p) * 15, l);
        float* oc = io.style_input + (int64_t)n * 45 * hw + p;
#pragma unroll
        for (int c = 0; c < 30; c++)
            store4(oc + c * hw, unit((float)byte_of(a, c)), unit((float)byte_of(a, 30 + c)), unit((float)byte_of(a, 60 + c)),
                   unit((float)byte_of(a, 90 + c)));
        // dataset.py:1160-1170: part 0 zeroed and the top rows of lower parts 1 and 3 (channels 3..5, 9..11); or rows ty : by of part 0
        const bool zero0 = s_kind == PG_ERASE_DROP_PART0 || (s_kind == PG_ERASE_BAND && y >= s_ty && y < s_by);
        const bool zero13 = y < s_rows;
#pragma unroll
        for (int c = 0; c < 15; c++) {
            const bool z = (c < 3) ? zero0 : ((c / 3 == 1 || c / 3 == 3) ? zero13 : false);
            const uint32_t k = z ? 0u : 0xffu;
            store4(oc + (30 + c) * hw, unit((float)(byte_of(l, c) & k)), unit((float)(byte_of(l, 15 + c) & k)), unit((float)(byte_of(l, 30 + c) & k)),
                   unit((float)(byte_of(l, 45 + c) & k)));
        }
    }
}

}  // namespace

PG_EXPORT int pg_train_fetch_abi_version(void) { return PG_ABI_VERSION; }

PG_EXPORT int pg_train_fetch(const pg_train_io* io, int n, int H, int W, int h, int w, void* stream) {
    if (!io || n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return PG_ERR_INVALID_ARG;
    const void* req[] = {io->image, io->pose, io->retain_mask, io->gt_parsing, io->denorm_upper, io->denorm_lower, io->norm_img, io->norm_img_lower,
                         io->skin, io->label, io->bound_rows, io->extents, io->erase, io->band_u, io->real_img, io->style_input, io->retain, io->pose_out,
                         io->denorm_upper_out, io->denorm_lower_out, io->upper_mask_out, io->lower_mask_out, io->gt_parsing_out};
    for (const void* p : req)
        if (!p) return PG_ERR_INVALID_ARG;
    if (W % 4 || w % 4) return PG_ERR_UNSUPPORTED;
    const void* u8[] = {io->image, io->pose, io->retain_mask, io->gt_parsing, io->random_mask, io->denorm_upper, io->denorm_lower, io->norm_img,
                        io->norm_img_lower};
    for (const void* p : u8)
        if (reinterpret_cast<uintptr_t>(p) & 3u) return PG_ERR_UNSUPPORTED;
    const void* f32[] = {io->real_img, io->style_input, io->retain, io->pose_out, io->denorm_upper_out, io->denorm_lower_out, io->upper_mask_out,
                         io->lower_mask_out, io->gt_parsing_out};
    for (const void* p : f32)
        if (!pg::aligned16(p)) return PG_ERR_UNSUPPORTED;
    if ((int64_t)H * W > 0x3fffffffLL || (int64_t)h * w > 0x3fffffffLL || n > 65535) return PG_ERR_TOO_LARGE;
    const int big = (int)(((int64_t)H * W / 4 + 255) / 256), small = (int)(((int64_t)h * w / 4 + 255) / 256);
    hipLaunchKernelGGL(train_fetch_kernel, dim3((unsigned)(big + small), (unsigned)n), dim3(256), 0, (hipStream_t)stream, *io, H, W, h, w, big);
    return pg::launch_status();
}
