// f0_pm.hip -- the "pm" f0 method (Praat's autocorrelation tracker) as a plan: three launches on the engine's 16 kHz input, then the pitch tail RMVPE uses
// (build_pitch_post, model_rmvpe.hip), fed as YIN feeds it.  DESIGN.md section 26
#include <cmath>

#include "engine_int.h"
#include "pm.hip.h"

namespace rvc {

// the normalised autocorrelation of the Hanning window at the lags 0 .. 352, in double, rounded to float once: the rounded table is part of the definition
std::vector<float> pm_rw_table()
{
    std::vector<float> t(PM_NLAG);
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < PM_NLAG; i++) {
        const double u = (double)i / PM_W;
        t[i] = (float)((1.0 - u) * (2.0 / 3.0 + std::cos(2.0 * pi * u) / 3.0) + std::sin(2.0 * pi * u) / (2.0 * pi));
    }
    return t;
}

static void check_pm_frames(int B, long long n, long long frame, int Tm)
{
    // (one reflection per side: every index the candidates' kernel forms lies in [0, frame))
    if (B < 1 || B > 65535 || Tm < 1 || Tm > 1024 || frame > n || frame < PM_PAD + 1 || (long long)(Tm - 1) * PM_HOP > frame || n > 0x7fffffffLL) throw ShapeError("pm: frame out of range");
}

void launch_pm_cand(hipStream_t s, int B, const float *audio, long long audio_bs, int n, int frame, int Tm, const float *rw, float *gpk, int *cn, float *cf, float *cs, float *cd)
{
    check_pm_frames(B, n, frame, Tm);
    if (!audio || !rw || !gpk || !cn || !cf || !cs || !cd || audio_bs < n) throw ShapeError("pm candidates: arrays");
    PmP q{};
    q.audio = audio; q.audio_bs = audio_bs; q.n = n; q.frame = frame; q.Tm = Tm; q.rw = rw; q.gpk = gpk; q.cn = cn; q.cf = cf; q.cs = cs; q.cd = cd;
    hipLaunchKernelGGL(pm_peak_kernel, dim3(B), dim3(256), 0, s, q);
    hipLaunchKernelGGL(pm_cand_kernel, dim3(Tm, B), dim3(PM_THREADS), 0, s, q);
}

void launch_pm_path(hipStream_t s, int B, int Tm, const int *cn, const float *cf, const float *cd, int *path, float *f0)
{
    if (B < 1 || B > 65535 || Tm < 1 || Tm > 1024 || !cn || !cf || !cd || !path || !f0) throw ShapeError("pm path: shape");
    PmP q{};
    q.Tm = Tm; q.cn = const_cast<int *>(cn); q.cf = const_cast<float *>(cf); q.cd = const_cast<float *>(cd); q.path = path; q.f0 = f0;
    hipLaunchKernelGGL(pm_path_kernel, dim3(B), dim3(64), 0, s, q);
}

// raw f0 [B][Tm] of the last f0_extractor_frame samples of each stream of pl.d_in ([B][L]), on RMVPE's frame grid: build_yin's contract, panics and refusals.
// An eager launch reads the caller's device buffer (Plan::cur_in) when there is one.
float *build_pm(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k)
{
    (void)e;
    const size_t fr = 5120 * ((frame16k + 800 - 1) / 5120 + 1) - 160;     // rmvpe.rs:256
    if (fr > L) throw PanicError("input shorter than f0_extractor_frame");
    const int Tm = (int)(1 + fr / 160);
    if (Tm % 32 != 0) throw PanicError("mel frame count is not a multiple of 32 (rmvpe.rs:229-233 branch)");
    if (Tm > 1024) throw ShapeError("f0 window too long");
    check_pm_frames(B, (long long)L, (long long)fr, Tm);
    pl.Tm = Tm;
    Arena &A = pl.arena;
    PmP q{};
    q.audio = pl.d_in; q.audio_bs = (long long)L; q.n = (int)L; q.frame = (int)fr; q.Tm = Tm;
    q.rw = A.upload(pm_rw_table());
    q.gpk = A.floats((size_t)B * 2);
    q.cn = (int *)A.alloc((size_t)B * Tm * sizeof(int));
    q.cf = A.floats((size_t)B * Tm * PM_NC); q.cs = A.floats((size_t)B * Tm * PM_NC); q.cd = A.floats((size_t)B * Tm * PM_NC);
    q.path = (int *)A.alloc((size_t)B * Tm * sizeof(int));
    q.f0 = A.floats((size_t)B * Tm);
    Plan *plp = &pl;
    pl.ops.push_back([=](hipStream_t s) { PmP q2 = q; if (plp->cur_in) q2.audio = plp->cur_in; hipLaunchKernelGGL(pm_peak_kernel, dim3(B), dim3(256), 0, s, q2); });
    add_stamp(pl, "pm.peak");
    pl.ops.push_back([=](hipStream_t s) { PmP q2 = q; if (plp->cur_in) q2.audio = plp->cur_in; hipLaunchKernelGGL(pm_cand_kernel, dim3(Tm, B), dim3(PM_THREADS), 0, s, q2); });
    add_stamp(pl, "pm.cand");
    pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(pm_path_kernel, dim3(B), dim3(64), 0, s, q); });
    add_stamp(pl, "pm.path");
    return q.f0;
}

}  // namespace rvc
