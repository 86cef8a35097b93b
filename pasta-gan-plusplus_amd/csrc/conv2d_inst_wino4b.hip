// Winograd F(4x4, 3x3), two-workgroups-per-CU form (conv2d_wino4b.h): the run-time-tail instantiations + dispatch.
// hipcc-flags: -fno-slp-vectorize
// (scalar fp32 transforms on purpose: packed fp32 VALU is slow beside MFMAs on gfx950)
#include "conv2d_wino4b.h"

namespace pgconv {
int launch_wino4b_spade(const ConvParams& p, hipStream_t s);      // conv2d_inst_wino4bs.hip
int launch_wino4b_plain(const ConvParams& p, hipStream_t s);      // conv2d_inst_wino4bs.hip
int launch_wino4b(const ConvParams& p, hipStream_t s) {
    if (wino4_declines(p, false)) return PG_ERR_UNSUPPORTED;      // no statistics tail in this form
    if (p.f.spade_x) return launch_wino4b_spade(p, s);
    if (!p.f.in_scale && !p.f.residual && !p.f.noise) return launch_wino4b_plain(p, s);
    return p.f.in_scale ? launch_wino4b_mode<1, W4_TAIL_ANY>(p, s) : launch_wino4b_mode<0, W4_TAIL_ANY>(p, s);
}
}  // namespace pgconv
