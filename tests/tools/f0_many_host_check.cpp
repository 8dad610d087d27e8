// f0_many_host_check.cpp -- where the f0 rows of many recordings land (obs_rvc_amd/csrc/convert_many_geometry.h: grid_off, many_grid_row)
// as a stand-alone CPU program, meant to be built with the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/tools/f0_many_host_check.cpp -o f0_many_host_check && ./f0_many_host_check
// It walks many small lists of file lengths with the lookup f0_export_many_kernel uses and exits non-zero on the first property that does not hold: the files'
// regions tile the grid arena, every row of every file is written by exactly one (global window, hop row), that pair is the one the single-file export names, and
// the rows a file's last, partial hop does not have are dropped instead of landing in the next file's region.  Nothing of the GPU is included.
#include "../../obs_rvc_amd/csrc/convert_many_geometry.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n  list=%ld F=%zu k=%zu C=%zu X=%zu rate=%zu\n", __FILE__, __LINE__, #c, lists, F, k, C, X, rate); return 1; } } while (0)

int main()
{
    using namespace rvc;
    struct Geo { size_t k, C, X, rate; };
    const Geo geos[] = {{2, 3, 2, 4800}, {2, 28, 3, 16000}, {3, 3, 1, 100}, {0, 0, 0, 48000}};
    long lists = 0, rows_walked = 0, dropped = 0;
    size_t F = 0, k = 0, C = 0, X = 0, rate = 0;
    unsigned long long seed = 0xD1B54A32D192ED03ull;
    auto rnd = [&seed]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    for (const Geo &ge : geos) {
        k = ge.k; C = ge.C; X = ge.X; rate = ge.rate;
        ConvertGeometry one;
        CHECK(convert_geometry(1, rate, k, C, X, &one) == nullptr);
        const size_t H = one.H;
        const size_t edges[] = {1, 2, 159, 160, 161, 160 * H - 1, 160 * H, 160 * H + 1, 320 * H, 320 * H + 1, 480 * H + 159, 160 * H * 7 + 5};
        const size_t n_edges = sizeof edges / sizeof edges[0];
        for (int rep = 0; rep < 1500; rep++) {
            F = 1 + (size_t)(rnd() % (rep % 8 == 0 ? 40 : 9));
            std::vector<size_t> n(F);
            for (size_t f = 0; f < F; f++) n[f] = rep % 3 == 0 ? 1 + (size_t)(rnd() % (160 * H * 4)) : edges[rnd() % n_edges];
            ConvertManyGeometry m;
            CHECK(convert_many_geometry(n.data(), F, rate, k, C, X, &m) == nullptr);
            lists++;
            // the regions tile the arena: offsets are the prefix sums of Nf_f = ceil(N_f / 160), whatever the model's rate
            const std::vector<long long> goff = m.grid_off();
            CHECK(goff.size() == F + 1 && goff[0] == 0);
            for (size_t f = 0; f < F; f++) CHECK(goff[f + 1] - goff[f] == (long long)((n[f] + 159) / 160) && goff[f + 1] > goff[f]);
            const size_t rows = (size_t)goff[F];
            std::vector<int> writes(rows, 0);
            std::vector<int> writer_g(rows, -1), writer_h(rows, -1);
            const int W = (int)m.windows_total();
            for (int g = 0; g < W; g++) {
                const int f = many_file_of(m.P.data(), (int)F, g), w = g - m.P[f];
                for (int h = 0; h < (int)H; h++) {
                    const long long at = many_grid_row(m.P.data(), goff.data(), (int)F, g, h, (int)H);
                    const long long row = (long long)w * (long long)H + h, Nf = goff[f + 1] - goff[f];
                    if (row >= Nf) { CHECK(at == -1); dropped++; continue; }      // the partial last hop: never the next file's first rows
                    CHECK(at == goff[f] + row && at >= goff[f] && at < goff[f + 1]);
                    writes[(size_t)at]++; writer_g[(size_t)at] = g; writer_h[(size_t)at] = h;
                }
            }
            for (size_t f = 0; f < F; f++)
                for (long long r = goff[f]; r < goff[f + 1]; r++) {
                    CHECK(writes[(size_t)r] == 1);
                    // ... by the (window, hop row) the single-file export names: row j of a file comes from its window j / H, hop row j % H
                    const long long j = r - goff[f];
                    CHECK(writer_g[(size_t)r] == m.P[f] + (int)(j / (long long)H) && writer_h[(size_t)r] == (int)(j % (long long)H));
                    rows_walked++;
                }
        }
    }
    printf("f0_many_host_check: %ld lists, %ld rows each written once, %ld rows of partial hops dropped: ok\n", lists, rows_walked, dropped);
    return 0;
}
