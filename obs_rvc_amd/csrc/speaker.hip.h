// speaker.hip.h -- run-time speaker selection: the one kernel that refolds the speaker conditioning into the live bias buffers of the synthesizer
// (DESIGN.md section 24).  Included by model_synth.hip only (a __global__ function lives in the one unit that launches it).
//
// The speaker enters the network as cond(g) = cond_w g + cond_b, a per-channel constant added to the pre-activations of every WaveNet in-layer of
// the flows and to dec_pre's output; the loader folds it into those layers' biases for g = sy.g.  With a speaker table on the device the same fold is
// one launch for any g = sum_i w_i emb_g[id_i] (n <= 8, i ascending, fp32):
//   bias[r] = base_b[r] + (cond_b[r] + sum_q cond_w[r][q] g[q])          for every model row r of every conditioned layer
// Every workgroup forms g in LDS (gin floats; n gin table reads, L2 hits after the first workgroup); every wave owns output rows, its lanes stride
// over q (coalesced reads of the row of cond_w), and the partial sums meet in wave_sum, a butterfly whose order is fixed: a bias depends on the mix and
// the weights, never on the grid, the wave that computed it or what ran before.  The result is stored with plain vector stores by lane 0 at the
// layer's position of row r: GLU-packed (glu_packed_row, the inverse of glu_pack_rows' map) for the in-layers -- to the plain copy and, when the
// flows are composed, to the composed twin: the same bits -- and r itself for dec_pre.
#pragma once
#include "engine_int.h"
#include "reduce.hip.h"

namespace rvc {

constexpr int SPK_WAVES = 4;            // waves (= rows in flight) per workgroup
constexpr int SPK_MAX_WGS = 512;        // 5 120 rows at full size: 2.5 rows per wave

__global__ __launch_bounds__(SPK_WAVES * 64) void speaker_fold_kernel(const SpeakerMix *mix, const float *emb, int n_spk, int gin, const SpeakerLayer *layers,
                                                                      int nlayers, int total_rows)
{
    extern __shared__ __attribute__((aligned(16))) float spk_g[];      // [gin]
    const int n = min(max(mix->n, 0), SPK_MAX_MIX);
    for (int q = threadIdx.x; q < gin; q += blockDim.x) {
        float a = 0.f;
        for (int i = 0; i < n; i++) {
            const int id = mix->id[i];
            if (id >= 0 && id < n_spk) a += mix->w[i] * emb[(size_t)id * gin + q];      // (the host has checked the ids: a second fence, not a path)
        }
        spk_g[q] = a;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = blockIdx.x * SPK_WAVES + wave; r < total_rows; r += gridDim.x * SPK_WAVES) {
        int l = 0;
        while (l + 1 < nlayers && r >= layers[l + 1].row0) l++;      // (wave-uniform: at most 17 layers)
        const SpeakerLayer L = layers[l];
        const int m = r - L.row0;
        if (m < 0 || m >= L.rows) continue;
        const float *cw = L.cond_w + (size_t)m * gin;
        float a = 0.f;
        for (int q = lane; q < gin; q += 64) a += cw[q] * spk_g[q];
        a = wave_sum(a);
        if (lane == 0) {
            const float v = L.base_b[m] + (L.cond_b[m] + a);
            const int p = L.glu_h ? glu_packed_row(m, L.glu_h) : m;
            L.dst0[p] = v;
            if (L.dst1) L.dst1[p] = v;
        }
    }
}

}  // namespace rvc
