// windows.hip.h -- what every windowed call on recordings shares (DESIGN.md sections 19, 28 to 31), included by f0_analyze.hip.h (engine.hip's unit): the
// upload of a call's signals and per-file tables, the gather of a batch's windows, the export of a batch's f0 rows, the high-pass launch and the silence gate
// over the files of a call.  A call packs the windows of its F recordings end to end (convert_many_geometry.h); a single recording is the call with F = 1, on
// the same kernels -- many_file_of then returns 0 without a loop iteration.
#pragma once
#include "convert_many_geometry.h"
#include "highpass.hip.h"
#include "silence.hip.h"

namespace rvc {

// the tables of a call on the device: the five per-file arrays in one allocation and the window prefix sums, copied before upload() returns
struct ManyDeviceTables {
    DevBuf<long long> ll; DevBuf<int> P;
    ManyTables t{};
    // sig_off / sig_n / out_off / out_n [F], goff [F + 1]
    void upload(const std::vector<int> &Pv, const std::vector<long long> &sig_off, const std::vector<long long> &sig_n, const std::vector<long long> &out_off,
                const std::vector<long long> &out_n, const std::vector<long long> &goff)
    {
        const size_t F = Pv.size() - 1;
        std::vector<long long> host(5 * F + 1);
        for (size_t f = 0; f < F; f++) { host[f] = sig_off[f]; host[F + f] = sig_n[f]; host[2 * F + f] = out_off[f]; host[3 * F + f] = out_n[f]; }
        for (size_t f = 0; f <= F; f++) host[4 * F + f] = goff[f];
        ll.alloc(5 * F + 1); P.alloc(F + 1);
        HIPCHK(hipMemcpy(ll.get(), host.data(), host.size() * sizeof(long long), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(P.get(), Pv.data(), (F + 1) * sizeof(int), hipMemcpyHostToDevice));
        t = ManyTables{P.get(), ll.get(), ll.get() + F, ll.get() + 2 * F, ll.get() + 3 * F, ll.get() + 4 * F, (int)F};
    }
    void upload(const ConvertManyGeometry &m)
    {
        const size_t F = m.files();
        std::vector<long long> sig_n(F), out_n(F);
        for (size_t f = 0; f < F; f++) { sig_n[f] = (long long)m.n[f]; out_n[f] = (long long)m.out_samples[f]; }
        upload(m.P, m.sig_off, sig_n, m.out_off, out_n, m.grid_off());
    }
};

// the signal arena of a call and its tables on the device, copied before it returns
static void many_upload(const float *const *pcm, const ConvertManyGeometry &m, DevBuf<float> *arena, ManyDeviceTables *tabs)
{
    std::vector<float> stage(m.sig_total());
    for (size_t f = 0; f < m.files(); f++) memcpy(stage.data() + m.sig_off[f], pcm[f], m.n[f] * sizeof(float));
    arena->alloc(m.sig_total());
    HIPCHK(hipMemcpy(arena->get(), stage.data(), stage.size() * sizeof(float), hipMemcpyHostToDevice));
    tabs->upload(m);
}

// the plan's batch input [S][n]: stream s gets global window g = j0 + s (win_of[j0 + s] under the silence gate) = window w of file f, samples
// [160 (w H - C), + n) of THAT file, zero outside [0, N_f) -- a sample of the neighbour file in the arena is never read; streams at or beyond nw (the padding
// of the call's last batch) get zeros
static __global__ __launch_bounds__(256) void gather_windows_kernel(const float *sig, ManyTables tabs, float *dst, int n, const int *__restrict__ win_of, int j0, int nw, int H, int C)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (i >= n) return;
    float v = 0.f;
    if (s < nw) {
        const int g = win_of ? win_of[j0 + s] : j0 + s, f = many_file_of(tabs.P, tabs.n_files, g), w = g - tabs.P[f];
        const long long src = 160LL * ((long long)w * H - C) + i;
        if (src >= 0 && src < tabs.sig_n[f]) v = sig[tabs.sig_off[f] + src];
    }
    dst[(long long)s * n + i] = v;
}

// gate: the silence gate's analysis of the call, or null; j0: the batch's first global window (gated: its first place), nw of the S streams hold a window
static void launch_gather_windows(hipStream_t st, const float *sig, const ManyTables &tabs, float *dst, size_t S, const SilenceWork *gate, size_t j0, int nw, const ConvertGeometry &g)
{
    hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)((g.n + 255) / 256), (unsigned)S), dim3(256), 0, st, sig, tabs, dst, (int)g.n,
                       gate ? (const int *)gate->win_of.get() : (const int *)nullptr, (int)j0, nw, (int)g.H, (int)g.C);
}

// after a batch: the rows f0 [S][Tm] of its windows onto the f0 grids of the call.  Hop rows [C, C + H) of stream s = global window g (as the gather's) =
// window w of file f go to rows [w H, min((w + 1) H, Nf_f)) of that file's region of the grid arena -- the last, partial hop of a file stops at its own end,
// and every row is written exactly once over the batches, no atomics.  Streams at or beyond nw write nothing.  Grid (ceil(H / 256), S)
static __global__ __launch_bounds__(256) void f0_export_many_kernel(const float *__restrict__ f0, int Tm, ManyTables tabs, const int *__restrict__ win_of, int j0, int nw, int H, int C,
                                                                    float *__restrict__ grid)
{
    const int h = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (h >= H || C + h >= Tm || s >= nw) return;
    const int g = win_of ? win_of[j0 + s] : j0 + s;
    const long long at = many_grid_row(tabs.P, tabs.goff, tabs.n_files, g, h, H);
    if (at >= 0) grid[at] = f0[(long long)s * Tm + C + h];
}

static void launch_f0_export_many(hipStream_t st, const float *f0, int Tm, const ManyTables &tabs, size_t S, const SilenceWork *gate, size_t j0, int nw, int H, int Cg, float *grid)
{
    hipLaunchKernelGGL(f0_export_many_kernel, dim3((unsigned)((H + 255) / 256), (unsigned)S), dim3(256), 0, st, f0, Tm, tabs, gate ? (const int *)gate->win_of.get() : (const int *)nullptr,
                       (int)j0, nw, H, Cg, grid);
}

// for rvc_debug_f0_override op 3 (debug.hip): the rows f0 [nw][Tm] of windows w0 .. of ONE recording onto its grid [Nf], through the launch above on a
// one-file table
void launch_f0_export(hipStream_t s, const float *f0, int Tm, int w0, int nw, int H, int C, float *grid, long long Nf)
{
    if (nw < 1 || H < 1) return;
    ManyDeviceTables tabs;
    tabs.upload({0, w0 + nw}, {0}, {0}, {0}, {0}, {0, Nf});
    launch_f0_export_many(s, f0, Tm, tabs.t, (size_t)nw, nullptr, (size_t)w0, nw, H, C, grid);
    HIPCHK(hipStreamSynchronize(s));      // (the tables go with this frame)
}

static void launch_highpass(rvc_engine *e, const float *d_x, size_t n, float *d_y)
{
    if (!e->hp_taps) {
        const std::vector<float> h = highpass_taps();
        e->hp_taps.alloc(h.size());
        HIPCHK(hipMemcpy(e->hp_taps.get(), h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (n > ((size_t)1 << 40)) throw ShapeError("highpass: signal too long");
    hipLaunchKernelGGL(highpass_fir_kernel, dim3((unsigned)((n + HP_TILE - 1) / HP_TILE)), dim3(HP_THREADS), 0, e->stream, d_x, (long long)n, (const float *)e->hp_taps.get(), d_y);
}
// each file of the arena on its own: rvc_highpass's bits, the zero extension per file
static void many_highpass(rvc_engine *e, const float *arena, const ConvertManyGeometry &m, float *filtered)
{
    for (size_t f = 0; f < m.files(); f++) launch_highpass(e, arena + m.sig_off[f], m.n[f], filtered + m.sig_off[f]);
}

// the silence gate (silence.hip.h) over the files of a call: every file measured on its own, the active windows of all files compacted in global window order;
// queued on st, returns behind the call's one read (synchronised).  zero_len: the samples of a stitch window (0: no stitch follows)
static void many_gate(hipStream_t st, const float *sig, const ConvertManyGeometry &m, double threshold_db, int hang_frames, size_t zero_len, SilenceWork *gate)
{
    const std::vector<long long> goff = m.grid_off();
    gate->begin(st, (size_t)goff.back(), m.windows_total(), threshold_db, hang_frames, zero_len);
    for (size_t f = 0; f < m.files(); f++)
        gate->queue_file(st, sig + m.sig_off[f], m.n[f], (size_t)(goff[f + 1] - goff[f]), (size_t)goff[f], m.windows[f], (size_t)m.P[f], m.g);
    gate->finish(st);
}
static inline bool silence_gate_on(const rvc_engine *e) { return e->sil_db > SILENCE_OFF_DB; }
static void silence_gate_report(rvc_engine *e, const SilenceWork &w)
{
    e->sil_info.run = w.A; e->sil_info.skipped = w.W - w.A; e->sil_info.loud = w.n_loud; e->sil_info.kept = w.n_kept; e->sil_info.ms = w.ms;
    e->sil_info.valid = true;
}

}  // namespace rvc
