// convert_many_geometry.h -- the host-only arithmetic of a windowed call on recordings: how the windows of F recordings of one geometry
// are laid end to end and cut into batches of S; rvc_convert's recording is the call with F = 1 (convert_many_single).  Plain C++, no HIP: every conversion
// and analysis calls it, and tests/tools/convert_many_host_check.cpp compiles it on its own under the sanitizers.  The functions the kernels share with the
// host, many_file_of and many_grid_row, are marked for both sides when a HIP compiler reads this file.
//
//   file f, N_f >= 1 samples:  Nf_f = ceil(N_f / 160),  W_f = ceil(Nf_f / H),  out_f = Nf_f zc            (convert_geometry.h, per file)
//   global window g = P_f + w,  P_f = W_0 + ... + W_{f-1},  0 <= w < W_f;   Wtot = P_F
//   batch i runs globals [i S, min((i + 1) S, Wtot)) on streams 0 ..; only the last batch is padded
// Files stay in the order given and windows in order: nothing is sorted.
#pragma once
#include "convert_geometry.h"

#include <algorithm>

#ifdef __HIPCC__
#define RVC_MANY_HD __host__ __device__
#else
#define RVC_MANY_HD
#endif

namespace rvc {

constexpr size_t CONVERT_MANY_MAX_FILES = 65536;
constexpr size_t CONVERT_MANY_MAX_WINDOWS = (size_t)1 << 30;      // a global window number is an int on the device
constexpr size_t CONVERT_MANY_MAX_OUT = (size_t)1 << 40;

// the file of global window g: the f with P[f] <= g < P[f + 1].  P [n_files + 1] is strictly increasing (every file has a window) and 0 <= g < P[n_files]
static inline RVC_MANY_HD int many_file_of(const int *P, int n_files, int g)
{
    int lo = 0, hi = n_files;      // P[lo] <= g < P[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (P[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// The f0 rows of many recordings: file f has Nf_f rows on its 10 ms grid, the grids lie end to end in one arena, goff [n_files + 1]
// their prefix sums.  Hop row h (0 <= h < H) of global window g = window w of file f is row w H + h of that file: -> its place in the arena, or -1 for a row
// at or beyond Nf_f (the file's last, partial hop: nothing lands in the next file's region)
static inline RVC_MANY_HD long long many_grid_row(const int *P, const long long *goff, int n_files, int g, int h, int H)
{
    const int f = many_file_of(P, n_files, g);
    const long long row = (long long)(g - P[f]) * H + h;
    return row < goff[f + 1] - goff[f] ? goff[f] + row : -1;
}

// the per-file tables of a call as the kernels read them, all indexed by file (windowed.hip.h uploads them): P [F + 1] window prefix sums, the file's place in
// the signal arena and in the output arena, goff [F + 1] the prefix sums of the files' f0 grids
struct ManyTables {
    const int *P; const long long *sig_off, *sig_n, *out_off, *out_n, *goff;
    int n_files;
};

// the packing of a call.  g: the shared window geometry (its Nf / windows / out_samples are file 0's and not used).  Per file: samples, windows, output
// samples; the prefix sums P (windows), sig_off (input samples) and out_off (output samples), each [n_files + 1]
struct ConvertManyGeometry {
    ConvertGeometry g;
    std::vector<size_t> n, windows, out_samples;
    std::vector<int> P;
    std::vector<long long> sig_off, out_off;
    size_t files() const { return n.size(); }
    size_t windows_total() const { return (size_t)P.back(); }
    size_t out_total() const { return (size_t)out_off.back(); }
    size_t sig_total() const { return (size_t)sig_off.back(); }
    size_t batches(size_t S) const { return (windows_total() + S - 1) / S; }
    // the f0 grid arena of the call: prefix sums [n_files + 1] of Nf_f = out_samples[f] / zc
    std::vector<long long> grid_off() const
    {
        std::vector<long long> o(files() + 1, 0);
        for (size_t f = 0; f < files(); f++) o[f + 1] = o[f] + (long long)(out_samples[f] / g.zc);
        return o;
    }
    // the files batch i of S streams touches: [first, last], a contiguous range
    void batch_files(size_t i, size_t S, int *first, int *last) const
    {
        const size_t g0 = i * S, g1 = std::min((i + 1) * S, windows_total());
        *first = many_file_of(P.data(), (int)files(), (int)g0);
        *last = many_file_of(P.data(), (int)files(), (int)(g1 - 1));
    }
};

// one recording of n samples with geometry g (convert_geometry's, of that n) as the call of one file it is
static inline ConvertManyGeometry convert_many_single(const ConvertGeometry &g, size_t n)
{
    ConvertManyGeometry m;
    m.g = g;
    m.n = {n}; m.windows = {g.windows}; m.out_samples = {g.out_samples};
    m.P = {0, (int)g.windows}; m.sig_off = {0, (long long)n}; m.out_off = {0, (long long)g.out_samples};
    return m;
}

// -> nullptr, or what is wrong with the arguments (k, context, crossfade: 0 = the defaults, as convert_geometry)
static inline const char *convert_many_geometry(const size_t *n16k, size_t n_files, size_t sample_rate, size_t k, size_t context, size_t crossfade, ConvertManyGeometry *m)
{
    if (n_files < 1 || n_files > CONVERT_MANY_MAX_FILES) return "convert_many: the number of recordings is outside [1, 65536]";
    if (!n16k) return "convert_many: null buffer";
    m->n.assign(n16k, n16k + n_files);
    m->windows.assign(n_files, 0); m->out_samples.assign(n_files, 0);
    m->P.assign(n_files + 1, 0); m->sig_off.assign(n_files + 1, 0); m->out_off.assign(n_files + 1, 0);
    size_t wtot = 0, otot = 0, stot = 0;
    for (size_t f = 0; f < n_files; f++) {
        if (n16k[f] == 0) return "convert_many: empty recording";
        ConvertGeometry g;
        if (const char *why = convert_geometry(n16k[f], sample_rate, k, context, crossfade, &g)) return why;
        if (f == 0) m->g = g;
        // (each term is at most 2^40, the sums are checked as they grow: nothing wraps)
        wtot += g.windows; otot += g.out_samples; stot += n16k[f];
        if (wtot > CONVERT_MANY_MAX_WINDOWS) return "convert_many: more than 2^30 windows in all";
        if (otot > CONVERT_MANY_MAX_OUT) return "convert_many: more than 2^40 output samples in all";
        m->windows[f] = g.windows; m->out_samples[f] = g.out_samples;
        m->P[f + 1] = (int)wtot; m->out_off[f + 1] = (long long)otot; m->sig_off[f + 1] = (long long)stot;
    }
    return nullptr;
}

}  // namespace rvc
