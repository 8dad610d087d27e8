// convert_host_check.cpp -- the file converter's host-only arithmetic (obs_rvc_amd/csrc/convert_geometry.h: window geometry, argument checks, high-pass taps)
// as a stand-alone CPU program, meant to be built with the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/tools/convert_host_check.cpp -o convert_host_check && ./convert_host_check
// It sweeps every (k, context, crossfade) the checks can accept or refuse at several rates and lengths, restates the invariants DESIGN.md section 19 derives
// and exits non-zero on the first one that does not hold.
#include "../../obs_rvc_amd/csrc/convert_geometry.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n  k=%zu C=%zu X=%zu rate=%zu n=%zu\n", __FILE__, __LINE__, #c, k, C, X, rate, n); return 1; } } while (0)

int main()
{
    using namespace rvc;
    const size_t rates[] = {0, 50, 4800, 16000, 32000, 40000, 44100, 48000, 48050, 102300, 102400, 384000, 400000};
    const size_t lens[] = {0, 1, 159, 160, 161, 160 * 233 + 77, 9600000, (size_t)1 << 40, ((size_t)1 << 40) * 160, ~(size_t)0};
    long accepted = 0, refused = 0;
    for (size_t k = 0; k <= 34; k++)
        for (size_t C = 0; C <= 520; C += (C < 60 ? 1 : 23))
            for (size_t X = 0; X <= 520; X += (X < 12 ? 1 : 37))
                for (size_t rate : rates)
                    for (size_t n : lens) {
                        ConvertGeometry g;
                        const char *why = convert_geometry(n, rate, k, C, X, &g);
                        const size_t ke = k ? k : CONVERT_DEFAULT_K, Ce = C ? C : 48, Xe = X ? X : 5;
                        const bool rate_ok = rate != 0 && rate % 100 == 0 && rate <= 384000;
                        const bool ok = ke >= 2 && ke <= 32 && Ce >= 3 && rate_ok && 2 * Ce + 2 * Xe + 1 <= 32 * ke - 1 && rate / 100 <= 1023 &&
                                        n / 160 + (n % 160 != 0) <= CONVERT_MAX_FRAMES;
                        CHECK((why == nullptr) == ok);
                        if (why) { CHECK(why[0] != 0); refused++; continue; }
                        accepted++;
                        CHECK(g.F == 32 * ke - 1 && g.n == 5120 * ke - 160 && g.sf == 5120 * (ke - 1) && g.skip_head == Ce && g.zc == rate / 100);
                        CHECK(5120 * ((g.sf + 799) / 5120 + 1) - 160 == g.n);                 // the f0 front end's window (rmvpe.rs:256) is the converter's
                        CHECK(1 + g.n / 160 == 32 * ke && 32 * ke <= 1024);                    // Tm
                        CHECK(g.H + 2 * Ce + Xe + 1 == g.F && g.H >= Xe && g.return_length == g.H + Xe + 1);
                        CHECK(g.skip_head + g.return_length <= g.F);                           // the feature slice (rvc.rs:155)
                        CHECK(1024 - g.F + g.skip_head >= 1024 - (32 * ke - 4));               // the pitch rows read are rows this window wrote (rvc.rs:172-176)
                        CHECK(1024 - g.F + g.skip_head + g.return_length <= 1024);
                        CHECK(g.Nf * 160 >= n && (g.Nf == 0 || (g.Nf - 1) * 160 < n));
                        CHECK(g.windows * g.H >= g.Nf && (g.windows == 0 || (g.windows - 1) * g.H < g.Nf));
                        CHECK(g.out_samples == g.Nf * g.zc);
                    }
    size_t k = 0, C = 0, X = 0, rate = 0, n = 0;
    const std::vector<float> h = highpass_taps();
    CHECK(h.size() == 2 * (size_t)HP_M + 1);
    double sum = 0;
    for (size_t j = 0; j < h.size(); j++) { sum += h[j]; CHECK(std::fabs(h[j] - h[h.size() - 1 - j]) < 1e-9); }
    CHECK(std::fabs(sum) < 1e-6 && h[HP_M] > 0.99 && h[HP_M] < 1.0 && std::fabs(h[0]) < 1e-12);
    printf("convert_host_check: %ld geometries accepted, %ld refused, %zu taps: ok\n", accepted, refused, h.size());
    return 0;
}
