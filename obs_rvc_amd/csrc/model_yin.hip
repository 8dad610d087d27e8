// model_yin.hip -- the YIN f0 method as a plan: one launch on the engine's 16 kHz input, then the pitch tail RMVPE uses (build_pitch_post, model_rmvpe.hip).  DESIGN.md section 11
#include "engine_int.h"
#include "yin.hip.h"

namespace rvc {

// raw f0 [B][Tm] of the last f0_extractor_frame samples of each stream of pl.d_in ([B][L]): the frames are the mel front end's (build_rmvpe), so Tm and the
// meaning of a row are RMVPE's and the pitch cache arithmetic behind it is unchanged.  An eager launch reads the caller's device buffer (Plan::cur_in) when there is one.
float *build_yin(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k)
{
    (void)e;
    const size_t fr = 5120 * ((frame16k + 800 - 1) / 5120 + 1) - 160;     // rmvpe.rs:256
    if (fr > L) throw PanicError("input shorter than f0_extractor_frame");
    const int Tm = (int)(1 + fr / 160);
    if (Tm % 32 != 0) throw PanicError("mel frame count is not a multiple of 32 (rmvpe.rs:229-233 branch)");
    if (Tm > 1024) throw ShapeError("f0 window too long");
    if (fr < YIN_PAD + 1 || (long long)(Tm - 1) * YIN_HOP > (long long)fr) throw ShapeError("YIN: frame out of range");   // (one reflection per side)
    pl.Tm = Tm;
    YinP yp{};
    yp.audio = pl.d_in; yp.audio_bs = (long long)L; yp.n = (int)L; yp.frame = (int)fr; yp.Tm = Tm;
    yp.f0 = pl.arena.floats((size_t)B * Tm);
    const dim3 grid(Tm, B);
    Plan *plp = &pl;
    pl.ops.push_back([=](hipStream_t s) { YinP y2 = yp; if (plp->cur_in) y2.audio = plp->cur_in; hipLaunchKernelGGL(yin_f0_kernel, grid, dim3(YIN_WAVES * 64), 0, s, y2); });
    add_stamp(pl, "yin.f0");
    return yp.f0;
}

}  // namespace rvc
