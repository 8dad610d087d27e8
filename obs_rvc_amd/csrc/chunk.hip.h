// chunk.hip.h -- the kernels engine.hip launches itself: the glue around a chunk (phone gather, feature extraction, the streams' chunk counters and
// state buckets) and the caller-side post-processing (RMS envelope mix, SOLA).  Included by engine.hip only.
#pragma once
#include "state.hip.h"
#include "protect.hip.h"
#include "reduce.hip.h"

namespace rvc {

// ------------------------------------------------------------------------------------
// small glue kernels
// ------------------------------------------------------------------------------------
// phone[c][r] = feats[min((skip_head + r) / 2, T - 1)][c]   (rvc.rs:99-109 + 155; Q2, Q8; the column rule: protect.hip.h phone_src_col)
static __global__ void gather_phone_kernel(const float *cv, int cv_cs, long long cv_bs, int C, int T, int skip_head, int R,
                                    float *phone, int ph_cs, long long ph_bs)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= C * R) return;
    int c = i / R, r = i - c * R;
    int s = phone_src_col(skip_head, r, T);
    phone[(long long)b * ph_bs + (long long)c * ph_cs + r] = cv[(long long)b * cv_bs + (long long)c * cv_cs + s];
}

// (1, 2T+1, C) output of RvcInfer::extract_feature (rvc.rs:99-109), contiguous
static __global__ void extract_feature_kernel(const float *cv, int cv_cs, int C, int T, float *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int T2 = 2 * T + 1;
    if (i >= T2 * C) return;
    int k = i / C, c = i - k * C;
    int s = k / 2; s = s < T - 1 ? s : T - 1;
    out[i] = cv[(long long)c * cv_cs + s];
}

// rvc_infer_batch_g: the states of one geometry bucket, gathered into a contiguous block (dir = 0) / scattered back (dir = 1); one workgroup per stream
static __global__ void state_gather_kernel(StreamState *all, StreamState *bucket, const int *idx, int dir)
{
    const int j = blockIdx.x, s = idx[j];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(dir ? bucket + j : all + s);
    uint32_t *dst = reinterpret_cast<uint32_t *>(dir ? all + s : bucket + j);
    for (int i = threadIdx.x; i < (int)(sizeof(StreamState) / 4); i += blockDim.x) dst[i] = src[i];
}

// bump the per-stream chunk counters after a call
// end of a chunk: the streams' chunk counters and the streams' status words, written straight into host-mapped memory (the host reads them after the call's one
// synchronisation: no copy kernel behind the chunk)
static __global__ void advance_chunk_kernel(StreamState *st, int B, int *host_status)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { st[b].chunk += 1; if (host_status) host_status[b] = st[b].status; }
}

// recover_retrieval (engine.hip): the chunk is issued again from the retrieval on, with the counter it had
static __global__ void rewind_chunk_kernel(StreamState *st, int B)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) st[b].chunk -= 1;
}

// ------------------------------------------------------------------------------------
// caller-side post-processing (reference: obs-rvc/src/rt_utils.rs:60-132, lib.rs:758-794)
// ------------------------------------------------------------------------------------
// rt_utils.rs:94-103: zero-pad frame/2, square, windowed mean (window frame, step hop), sqrt.  One workgroup per frame.
// (all post-processing kernels take a stream index in blockIdx.y -- blockIdx.x for post_sola_kernel -- and per-stream strides)
// The envelope is evaluated in f64 from the f32 samples and rounded once, where the mixed sample is stored: the result is the correctly rounded
// value of the definition, which no ordering of f32 roundings guarantees (DESIGN.md "Post-processing and resamplers: what is tested"; a few
// dozen values per stream and chunk: the cost is not measurable).  The tracks stay f64 between the two kernels.
static __global__ __launch_bounds__(256) void post_rms_kernel(const float *y, int n, int frame, int hop, double *out, long long y_bs, long long out_bs)
{
    __shared__ double red[256];
    y += blockIdx.y * y_bs; out += blockIdx.y * out_bs;
    const int f = blockIdx.x, pad = frame / 2;
    double s = 0.0;
    for (int j = threadIdx.x; j < frame; j += 256) {
        int q = f * hop + j - pad;
        const double v = (q >= 0 && q < n) ? (double)y[q] : 0.0;
        s += v * v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[f] = sqrt(red[0] / (double)frame);
}
// rt_utils.rs:105-117 evaluated at one index of the (size)-point output
__device__ __forceinline__ double lerp_align_corners_at(const double *in, int n_in, int size, int i)
{
    const double step = (double)(n_in - 1) / (double)(size - 1);
    const double idx = (double)i * step;
    int fl = (int)floor(idx), ce = (int)ceil(idx);
    fl = fl < 0 ? 0 : (fl > n_in - 1 ? n_in - 1 : fl);
    ce = ce < 0 ? 0 : (ce > n_in - 1 ? n_in - 1 : ce);
    const double fr = idx - (double)fl;
    return in[fl] * (1.0 - fr) + in[ce] * fr;
}
// rt_utils.rs:119-132
// mix_power_v: per-stream exponent (or nullptr: mix_power for every stream); an exponent of 0 leaves the stream untouched (pow(x, 0) = 1)
static __global__ void post_mix_kernel(float *out, int n, const double *r1, int n1, const double *r2, int n2, float mix_power, long long out_bs, long long r_bs, const float *mix_power_v)
{
    if (mix_power_v) mix_power = mix_power_v[blockIdx.y];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out += blockIdx.y * out_bs; r1 += blockIdx.y * r_bs; r2 += blockIdx.y * r_bs;
    const double a = lerp_align_corners_at(r1, n1, n + 1, i);
    const double b = fmax(lerp_align_corners_at(r2, n2, n + 1, i), (double)1e-3f);       // (the reference's floor is the f32 constant)
    out[i] = (float)((double)out[i] * pow(a / b, (double)mix_power));
}
// rt_utils.rs:60-90 + lib.rs:768-794 in one workgroup: normalised cross-correlation over search+1 lags (last maximum wins),
// sin^2 crossfade with the previous tail, new tail saved, first `frame` samples returned.
// normalised cross-correlation of get_sola_offset (rt_utils.rs:60-77), one wave per lag: cor[l] = <out[l..], sola> / sqrt(<out[l..], out[l..]> + 1e-8)
// with f64 accumulation (the reference's FFT convolution carries f32 rounding noise of the same order as an f32 direct sum)
// (one lag by one whole wave, every lane gets the value: shared with the file converter's offset chain, stitch.hip.h, which must pick the same offsets)
__device__ __forceinline__ float sola_corr_lag(const float *out_l, const float *sola, int sola_len, int lane)
{
    double nom = 0.0, den = 0.0;
    for (int j = lane; j < sola_len; j += 64) { const double v = (double)out_l[j]; nom += v * (double)sola[j]; den += v * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nom += __shfl_xor(nom, o, 64); den += __shfl_xor(den, o, 64); }
    return (float)nom / sqrtf((float)den + 1e-8f);
}
static __global__ __launch_bounds__(256) void post_sola_corr_kernel(const float *output, const float *sola, int sola_len, int search, float *cor,
                                                             long long out_bs, long long sola_bs, long long cor_bs)
{
    const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l > search) return;
    output += blockIdx.y * out_bs; sola += blockIdx.y * sola_bs; cor += blockIdx.y * cor_bs;
    const float c = sola_corr_lag(output + l, sola, sola_len, lane);
    if (lane == 0) cor[l] = c;
}
// arg-max over cor[0 .. search] with the reference's tie rule: the LAST maximum wins (rt_utils.rs:79-88)
__device__ __forceinline__ int sola_argmax_last(const float *cor, int search)
{
    int best = 0; float bv = cor[0];
    for (int l = 1; l <= search; l++) if (!(bv > cor[l])) { best = l; bv = cor[l]; }
    return best;
}
// sample i of the sin^2 crossfade of the new segment `o` with the saved tail `s` over sola_len samples (lib.rs:768-781)
__device__ __forceinline__ float sola_fade(float o, float s, int i, int sola_len)
{
    const float x = sola_len > 1 ? (float)i / (float)(sola_len - 1) : 0.f;
    const float sn = sinf(x * 0.5f * 3.14159265358979323846f);
    const float fi = sn * sn, fo = 1.0f - fi;
    return o * fi + s * fo;
}

// arg-max with the reference's tie rule (the LAST maximum wins, rt_utils.rs:79-88), sin^2 crossfade with the previous tail, tail save and
// frame extraction (lib.rs:768-794).  mode_v / mode_all: the crossfade of a stream (per stream, or one value for all when mode_v is NULL)
static __global__ __launch_bounds__(1024) void post_sola_kernel(float *output, float *sola, int sola_len, int search, int frame, float *frame_out, int *offset_out,
                                                         const float *cor_g, long long out_bs, long long sola_bs, long long frame_bs, long long cor_bs,
                                                         const int *mode_v = nullptr, int mode_all = 0, float *pv_a = nullptr, long long pva_bs = 0)
{
    __shared__ float cor[1024];
    __shared__ int s_off;
    const int t = threadIdx.x;
    output += blockIdx.x * out_bs; sola += blockIdx.x * sola_bs; frame_out += blockIdx.x * frame_bs; cor_g += blockIdx.x * cor_bs; offset_out += blockIdx.x;
    for (int l = t; l <= search; l += 1024) cor[l] = cor_g[l];
    __syncthreads();
    if (t == 0) {
        const int best = sola_argmax_last(cor, search);
        s_off = best; *offset_out = best;
    }
    __syncthreads();
    float *o = output + s_off;
    // a phase-vocoder stream (crossfade.hip.h) keeps the segment unblended and hands the old tail to the kernels behind this one, which
    // write the blend over output, frame and tail
    if ((mode_v ? mode_v[blockIdx.x] : mode_all) == 1) {
        for (int i = t; i < sola_len; i += 1024) pv_a[blockIdx.x * pva_bs + i] = sola[i];
    } else {
        for (int i = t; i < sola_len; i += 1024) o[i] = sola_fade(o[i], sola[i], i, sola_len);
    }
    __syncthreads();
    for (int i = t; i < sola_len; i += 1024) sola[i] = o[frame + i];
    for (int i = t; i < frame; i += 1024) frame_out[i] = o[i];
}

}  // namespace rvc
