// resample_host_check.cpp -- the host-only arithmetic of the whole-signal converter and of the volume envelope (obs_rvc_amd/csrc/resample_geometry.h,
// formant_table.h: ratio, filter width, output length, argument checks, the compact filter table) as a stand-alone CPU program, meant to be built with the
// sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/tools/resample_host_check.cpp -o resample_host_check && ./resample_host_check
// It sweeps rate pairs and lengths, restates what DESIGN.md section 20 derives for every accepted case and exits non-zero on the first one that does not hold.
#include "../../obs_rvc_amd/csrc/resample_geometry.h"

#include <cstdio>
#include <cstdlib>
#include <map>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n  rate_in=%zu rate_out=%zu n=%zu\n", __FILE__, __LINE__, #c, ri, ro, n); return 1; } } while (0)

struct Compact { std::vector<int> kb; int w = 0, Kt = 0; };

int main()
{
    using namespace rvc;
    const size_t rates[] = {0, 1, 2, 3, 147, 160, 441, 4410, 4800, 8000, 16000, 22050, 32000, 44100, 48000, 96000, 2048, 2047, 2049, 4099, (size_t)2048 * 4800, ~(size_t)0};
    const size_t lens[] = {0, 1, 2, 7, 159, 440, 441, 1000, 5003, 9600000, (size_t)1 << 40, ((size_t)1 << 40) + 1, ~(size_t)0};
    std::map<std::pair<size_t, size_t>, Compact> tables;
    long accepted = 0, refused = 0;
    for (size_t ri : rates)
        for (size_t ro : rates)
            for (size_t n : lens) {
                ResampleGeometry g;
                const char *why = resample_geometry(ri, ro, n, &g);
                const size_t d = ri && ro ? formant_gcd(ri, ro) : 1;
                const bool ok = ri != 0 && ro != 0 && ri / d <= 2048 && ro / d <= 2048 && n >= 1 && n <= (size_t)1 << 40;
                CHECK((why == nullptr) == ok);
                if (why) { CHECK(why[0] != 0); refused++; continue; }
                accepted++;
                CHECK(g.o * d == ri && g.n * d == ro && formant_gcd(g.o, g.n) == 1);
                CHECK(g.K == 2 * g.w + g.o && (double)g.w >= 6.0 * (double)g.o / (0.99 * (double)std::min(g.o, g.n)) && g.w >= 7);
                // N_out = ceil(N_in n / o), in 128-bit arithmetic
                const unsigned __int128 p = (unsigned __int128)n * g.n;
                CHECK((unsigned __int128)g.n_out * g.o >= p && (unsigned __int128)(g.n_out - 1) * g.o < p && g.n_out >= 1);
                Compact &c = tables[{g.o, g.n}];
                if (c.kb.empty()) {
                    if (g.o == g.n) { c.kb.assign(1, 0); c.Kt = 1; }      // a copy: no table
                    else {
                        std::vector<float> ht;
                        formant_table_compact(g.o, g.n, ht, c.kb, &c.w, &c.Kt);
                        CHECK((size_t)c.w == g.w && c.kb.size() == g.n && ht.size() == g.n * (size_t)c.Kt && c.Kt >= 1 && (size_t)c.Kt <= g.K);
                        std::vector<float> h; size_t w, K;
                        formant_table(g.o, g.n, h, &w, &K);
                        CHECK(w == g.w && K == g.K && h.size() == g.n * K);
                        for (size_t j = 0; j < g.n; j++) {
                            // every compact row's span lies inside [0, K); beyond its nonzero taps it holds zeros, and nothing outside the span is nonzero
                            CHECK(c.kb[j] >= 0 && (size_t)c.kb[j] < K);
                            size_t last = 0;
                            for (size_t k = 0; k < K; k++) {
                                const bool in = k >= (size_t)c.kb[j] && k < (size_t)c.kb[j] + c.Kt;
                                if (h[j * K + k] != 0.f) { CHECK(in); last = k; }
                                if (in) CHECK(ht[j * c.Kt + (k - c.kb[j])] == h[j * K + k]);
                            }
                            CHECK(last < K);
                            for (int t = 0; t < c.Kt; t++) if ((size_t)c.kb[j] + t >= K) CHECK(ht[j * c.Kt + t] == 0.f);
                        }
                    }
                }
                if (g.o == g.n) { CHECK(g.n_out == n); continue; }
                // the input span of the first and of the last output, clipped to the signal, lies inside [0, N_in) and is not empty: output m = i n + j reads
                // x[i o + k - w], k in [kb[j], kb[j] + Kt) below K
                for (size_t m : {(size_t)0, g.n_out - 1}) {
                    const size_t i = m / g.n, j = m % g.n;
                    const __int128 lo = (__int128)i * g.o + c.kb[j] - (__int128)g.w;
                    const __int128 hi = (__int128)i * g.o + std::min<size_t>((size_t)c.kb[j] + c.Kt, g.K) - (__int128)g.w;      // exclusive
                    const __int128 a = lo < 0 ? 0 : lo, b = hi > (__int128)n ? (__int128)n : hi;
                    CHECK(a >= 0 && b <= (__int128)n && a < b);
                }
            }
    size_t ri = 0, ro = 0, n = 0;
    // the volume envelope's frames
    long env = 0;
    for (size_t rate : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)99, (size_t)201, (size_t)4800, (size_t)16000, (size_t)1 << 20, ((size_t)1 << 20) + 1, ~(size_t)0})
        for (size_t len : lens) {
            ri = rate; n = len;
            RmsGeometry r;
            const char *why = change_rms_geometry(len, rate, &r);
            CHECK((why == nullptr) == (rate >= 2 && rate <= (size_t)1 << 20 && len >= 1 && len <= (size_t)1 << 30));
            if (why) continue;
            env++;
            CHECK(r.hop == rate / 2 && r.L == 2 * r.hop && r.L <= rate && r.F == 1 + len / r.hop);
            CHECK((r.F - 1) * r.hop <= len && r.F * r.hop > len);          // the last frame's centre is the last hop boundary inside the signal
            CHECK((r.F - 1) * r.hop + r.L <= len + r.L && r.F < ((size_t)1 << 31) && len + r.L < ((size_t)1 << 31));      // frames stay inside the padded signal; ints hold them
        }
    CHECK(change_rms_rate_ok(0.0) && change_rms_rate_ok(1.0) && change_rms_rate_ok(0.25) && !change_rms_rate_ok(-0.01) && !change_rms_rate_ok(1.01) && !change_rms_rate_ok(std::nan("")));
    printf("resample_host_check: %ld geometries accepted, %ld refused, %zu tables, %ld envelope geometries: ok\n", accepted, refused, tables.size(), env);
    return 0;
}
