// convert_many_host_check.cpp -- the packing of rvc_convert_many (obs_rvc_amd/csrc/convert_many_geometry.h: windows of several recordings laid end to end,
// batches of S, the signal and output arenas) as a stand-alone CPU program, meant to be built with the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/tools/convert_many_host_check.cpp -o convert_many_host_check && ./convert_many_host_check
// It walks the tables over many small lists of file lengths and stream counts, with the lookup the kernels use (many_file_of), and exits non-zero on the
// first property DESIGN.md section 29 states that does not hold.  Nothing of the GPU is included.
#include "../../obs_rvc_amd/csrc/convert_many_geometry.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n  list=%ld F=%zu S=%zu k=%zu C=%zu X=%zu rate=%zu\n", __FILE__, __LINE__, #c, lists, F, S, k, C, X, rate); return 1; } } while (0)

int main()
{
    using namespace rvc;
    struct Geo { size_t k, C, X, rate; };
    const Geo geos[] = {{2, 3, 2, 4800}, {2, 28, 3, 4800}, {3, 3, 1, 100}, {0, 0, 0, 48000}};
    long lists = 0, refused = 0, windows_walked = 0, batches_walked = 0;
    size_t F = 0, S = 0, k = 0, C = 0, X = 0, rate = 0;
    unsigned long long seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&seed]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    for (const Geo &ge : geos) {
        k = ge.k; C = ge.C; X = ge.X; rate = ge.rate;
        ConvertGeometry one;
        CHECK(convert_geometry(1, rate, k, C, X, &one) == nullptr);
        const size_t H = one.H, zc = one.zc;
        // lengths at the edges of a frame and of a hop, and a few long ones
        const size_t edges[] = {1, 2, 159, 160, 161, 160 * H - 1, 160 * H, 160 * H + 1, 320 * H, 320 * H + 1, 480 * H + 159, 160 * H * 7 + 5};
        const size_t n_edges = sizeof edges / sizeof edges[0];
        for (int rep = 0; rep < 4000; rep++) {
            F = 1 + (size_t)(rnd() % (rep % 8 == 0 ? 40 : 9));
            std::vector<size_t> n(F);
            for (size_t f = 0; f < F; f++) n[f] = rep % 3 == 0 ? 1 + (size_t)(rnd() % (160 * H * 4)) : edges[rnd() % n_edges];
            ConvertManyGeometry m;
            const char *why = convert_many_geometry(n.data(), F, rate, k, C, X, &m);
            S = 0;
            CHECK(why == nullptr);
            lists++;
            CHECK(m.files() == F && m.P.size() == F + 1 && m.sig_off.size() == F + 1 && m.out_off.size() == F + 1 && m.P[0] == 0 && m.sig_off[0] == 0 && m.out_off[0] == 0);
            // per file: rvc_convert_geometry's numbers; prefix sums; output regions tile the output without overlap, signal regions the arena
            for (size_t f = 0; f < F; f++) {
                ConvertGeometry g;
                CHECK(convert_geometry(n[f], rate, k, C, X, &g) == nullptr);
                CHECK(m.windows[f] == g.windows && m.windows[f] >= 1 && m.out_samples[f] == g.out_samples && m.n[f] == n[f]);
                CHECK((size_t)(m.P[f + 1] - m.P[f]) == g.windows);
                CHECK((size_t)(m.out_off[f + 1] - m.out_off[f]) == g.out_samples && (size_t)(m.sig_off[f + 1] - m.sig_off[f]) == n[f]);
                // the windows of a file cover its output: (W - 1) H zc < out <= W H zc, so the last window writes the last sample and no window starts beyond it
                CHECK((g.windows - 1) * H * zc < g.out_samples && g.out_samples <= g.windows * H * zc);
                // one recording as the call of one file: what convert_many_geometry makes of the list {n_f}, table for table
                ConvertManyGeometry one_file, single = convert_many_single(g, n[f]);
                CHECK(convert_many_geometry(&n[f], 1, rate, k, C, X, &one_file) == nullptr);
                CHECK(single.files() == 1 && single.n == one_file.n && single.windows == one_file.windows && single.out_samples == one_file.out_samples);
                CHECK(single.P == one_file.P && single.sig_off == one_file.sig_off && single.out_off == one_file.out_off && single.grid_off() == one_file.grid_off());
                CHECK(single.g.Nf == g.Nf && single.g.n == g.n && single.g.H == g.H && single.g.C == g.C && single.g.zc == g.zc && single.batches(3) == (g.windows + 2) / 3);
                CHECK(single.grid_off().size() == 2 && single.grid_off()[1] == (long long)g.Nf && many_file_of(single.P.data(), 1, (int)g.windows - 1) == 0);
            }
            // goff, the sixth table: prefix sums of Nf_f; the hop rows of a file's windows tile its region of the grid arena, each row once, none beyond it
            {
                const std::vector<long long> goff = m.grid_off();
                CHECK(goff.size() == F + 1 && goff[0] == 0);
                std::vector<int> hits((size_t)goff[F], 0);
                for (size_t f = 0; f < F; f++) {
                    CHECK((size_t)(goff[f + 1] - goff[f]) == m.out_samples[f] / zc && goff[f + 1] > goff[f]);
                    for (int gw = m.P[f]; gw < m.P[f + 1]; gw++)
                        for (size_t h = 0; h < H; h++) {
                            const long long at = many_grid_row(m.P.data(), goff.data(), (int)F, gw, (int)h, (int)H);
                            CHECK(at == -1 || (at >= goff[f] && at < goff[f + 1]));
                            CHECK((at == -1) == ((long long)(gw - m.P[f]) * (long long)H + (long long)h >= goff[f + 1] - goff[f]));
                            if (at >= 0) hits[(size_t)at]++;
                        }
                }
                for (int c : hits) CHECK(c == 1);
            }
            const size_t W = m.windows_total();
            CHECK(m.out_total() == (size_t)m.out_off[F] && m.sig_total() == (size_t)m.sig_off[F]);
            // every global window maps to exactly one (f, w), in file order then window order
            {
                size_t g = 0;
                for (size_t f = 0; f < F; f++)
                    for (size_t w = 0; w < m.windows[f]; w++, g++) {
                        const int ff = many_file_of(m.P.data(), (int)F, (int)g);
                        CHECK((size_t)ff == f && (size_t)((int)g - m.P[ff]) == w);
                        windows_walked++;
                    }
                CHECK(g == W);
            }
            // batches: contiguous in globals and in files, only the last one short, every file's windows of a batch one contiguous run
            for (size_t Sv : {(size_t)1, (size_t)2, (size_t)3, (size_t)8, (size_t)32, W, W + 1}) {
                S = Sv;
                const size_t B = m.batches(S);
                CHECK(B == (W + S - 1) / S && B >= 1);
                size_t seen = 0; int prev_last = 0;
                for (size_t b = 0; b < B; b++) {
                    const size_t g0 = b * S, g1 = std::min((b + 1) * S, W);
                    CHECK(g1 > g0 && (b + 1 == B || g1 - g0 == S));
                    int first = -1, last = -1;
                    m.batch_files(b, S, &first, &last);
                    CHECK(first >= 0 && last >= first && (size_t)last < F);
                    CHECK(b == 0 ? first == 0 : (first == prev_last || first == prev_last + 1));      // nothing skipped between batches
                    // what the chain kernel's workgroups walk: file f's globals [max(P_f, g0), min(P_{f+1}, g1)) -- non-empty, disjoint, covering the batch
                    size_t covered = 0;
                    for (int f = first; f <= last; f++) {
                        const size_t lo = std::max((size_t)m.P[f], g0), hi = std::min((size_t)m.P[f + 1], g1);
                        CHECK(hi > lo);
                        CHECK(f == first ? lo == g0 : lo == (size_t)m.P[f]);
                        covered += hi - lo;
                    }
                    CHECK(covered == g1 - g0);
                    CHECK((size_t)m.P[first] <= g0 && g1 <= (size_t)m.P[last + 1]);
                    seen += g1 - g0; prev_last = last; batches_walked++;
                }
                CHECK(seen == W && (size_t)prev_last == F - 1);
            }
        }
    }
    // refusals: no file, too many, an empty one anywhere, a bad geometry, a null table; the totals
    {
        k = 2; C = 3; X = 2; rate = 4800; S = 0;
        ConvertManyGeometry m;
        std::vector<size_t> n(CONVERT_MANY_MAX_FILES + 1, 160);
        F = 0; CHECK(convert_many_geometry(n.data(), 0, rate, k, C, X, &m) != nullptr); refused++;
        F = n.size(); CHECK(convert_many_geometry(n.data(), n.size(), rate, k, C, X, &m) != nullptr); refused++;
        F = CONVERT_MANY_MAX_FILES; CHECK(convert_many_geometry(n.data(), F, rate, k, C, X, &m) == nullptr && m.windows_total() == F && m.out_total() == F * 48);
        F = 3;
        for (size_t z = 0; z < 3; z++) { size_t v[3] = {160, 160, 160}; v[z] = 0; CHECK(convert_many_geometry(v, 3, rate, k, C, X, &m) != nullptr); refused++; }
        CHECK(convert_many_geometry(nullptr, 1, rate, k, C, X, &m) != nullptr); refused++;
        CHECK(convert_many_geometry(n.data(), 3, rate, 1, C, X, &m) != nullptr); refused++;
        CHECK(convert_many_geometry(n.data(), 3, 4850, k, C, X, &m) != nullptr); refused++;
        const size_t per = 160 * 54 * ((size_t)1 << 14);      // 2^14 windows a file; zc = 1 keeps the outputs under 2^40
        std::fill(n.begin(), n.end(), per);
        F = CONVERT_MANY_MAX_FILES; rate = 100;
        CHECK(convert_many_geometry(n.data(), F, rate, k, C, X, &m) == nullptr && m.windows_total() == CONVERT_MANY_MAX_WINDOWS && m.P[F] > 0);
        n[F - 1] = per + 1;
        CHECK(convert_many_geometry(n.data(), F, rate, k, C, X, &m) != nullptr); refused++;
        rate = 48000; k = 0; C = 0; X = 0; F = 4;
        const size_t frames = CONVERT_MANY_MAX_OUT / 480 / 4 + 1;
        size_t v[4] = {160 * frames, 160 * frames, 160 * frames, 160 * frames};
        CHECK(convert_many_geometry(v, 4, rate, k, C, X, &m) != nullptr); refused++;
        CHECK(convert_many_geometry(v, 3, rate, k, C, X, &m) == nullptr && m.out_total() == 3 * frames * 480);
        v[0] = ~(size_t)0;      // a length no recording has: refused by the first file's own check, nothing wraps
        CHECK(convert_many_geometry(v, 4, rate, k, C, X, &m) != nullptr); refused++;
    }
    printf("convert_many_host_check: %ld lists accepted, %ld refused, %ld windows and %ld batches walked: ok\n", lists, refused, windows_walked, batches_walked);
    return 0;
}
