// Winograd F(4x4, 3x3) instantiations (own translation units: see conv2d_kernel.h on build time): the run-time-tail fallbacks + dispatch.
// hipcc-flags: -fno-slp-vectorize
// (scalar fp32 transforms on purpose: packed fp32 VALU is slow beside MFMAs on gfx950)
#include "conv2d_wino4.h"

namespace pgconv {
int launch_wino4_spade(const ConvParams& p, hipStream_t s);      // conv2d_inst_wino4s.hip
int launch_wino4_plain(const ConvParams& p, hipStream_t s);      // conv2d_inst_wino4s.hip
int launch_wino4_stats(const ConvParams& p, hipStream_t s);      // conv2d_inst_wino4t.hip
int launch_wino4(const ConvParams& p, hipStream_t s) {
    if (wino4_declines(p, true)) return PG_ERR_UNSUPPORTED;
    static const bool split = [] { const char* e = getenv("PG_WINO4_TAILS"); return e ? atoi(e) != 0 : true; }();      // A/B switch: 0 = the run-time tail for everything but SPADE
    if (p.f.spade_x) return launch_wino4_spade(p, s);
    // (residual-only and modulated + noise instantiations were built and measured too: +1 % and -1 ... +5 % against the run-time tail -- not kept)
    if (p.f.stats_partial) return launch_wino4_stats(p, s);
    if (split && !p.f.in_scale && !p.f.residual && !p.f.noise) return launch_wino4_plain(p, s);
    return p.f.in_scale ? launch_wino4_mode<1, W4_TAIL_ANY>(p, s) : launch_wino4_mode<0, W4_TAIL_ANY>(p, s);
}
}  // namespace pgconv
