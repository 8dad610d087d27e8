// model_synth.hip -- the synthesizer (text encoder, prior sample, flows, NSF source, HiFiGAN decoder) as a plan (reference: rvc/src/rvc.rs:182-214, ort::Session::run at rvc.rs:195)
#include "engine_int.h"
#include "synth.hip.h"
#include "speaker.hip.h"

namespace rvc {

// ------------------------------- the model as loaded (struct ModelSY: engine_int.h) ------------------------------------------
template <typename T> void glu_pack_rows(const T *w, const float *bias, int H, size_t K, std::vector<float> &wp, std::vector<float> &bp)
{
    if (H % 8 != 0) throw std::runtime_error("GLU-gated layer: channel count must be a multiple of 8");
    wp.resize((size_t)2 * H * K); bp.resize((size_t)2 * H);
    for (int r = 0; r < 2 * H; r++) {
        const int src = glu_model_row(r, H);
        for (size_t q = 0; q < K; q++) wp[(size_t)r * K + q] = (float)w[(size_t)src * K + q];
        bp[r] = bias[src];
    }
}
template void glu_pack_rows<float>(const float *, const float *, int, size_t, std::vector<float> &, std::vector<float> &);
template void glu_pack_rows<double>(const double *, const float *, int, size_t, std::vector<float> &, std::vector<float> &);      // (compose_flows)
ModelSY::ModelSY(const Blob &b)
{
    phone_dim = b.icfg("phone_dim"); hidden = b.icfg("hidden"); inter = b.icfg("inter"); filter = b.icfg("filter"); heads = b.icfg("heads");
    enc_layers = b.icfg("enc_layers"); enc_k = b.icfg("enc_k"); window = b.icfg("window"); flow_n = b.icfg("flow_n");
    wn_layers = b.icfg("wn_layers"); wn_k = b.icfg("wn_k"); gin = b.icfg("gin"); up_init = b.icfg("up_init"); n_ups = b.icfg("n_ups");
    n_rb = b.icfg("n_rb"); n_rbd = b.icfg("n_rbd"); sr = b.icfg("sr");
    has_f0 = b.icfg_or("f0", 1) != 0;
    for (int i = 0; i < n_ups; i++) { up_rate[i] = b.icfg(fmt("up_rate%d", i)); up_kernel[i] = b.icfg(fmt("up_kernel%d", i)); }
    for (int j = 0; j < n_rb; j++) rb_k[j] = b.icfg(fmt("rb_k%d", j));
    for (int m = 0; m < n_rbd; m++) rb_d[m] = b.icfg(fmt("rb_d%d", m));
    auto own = [&](const std::string &n) { float *p = dv(b, n); owned.push_back(p); return p; };
    const int H = hidden, G = gin;
    const float *g = b.w("sy.g");
    phone = prep_conv(b.w("sy.enc.phone.w"), b.w("sy.enc.phone.b"), H, phone_dim, 1, 1);
    if (has_f0) pitch_emb = own("sy.enc.pitch_emb");
    for (int l = 0; l < enc_layers; l++) {
        Layer L;
        std::vector<float> w((size_t)3 * H * H), bb((size_t)3 * H);
        const char *nm[3] = {"q", "k", "v"};
        for (int j = 0; j < 3; j++) {
            memcpy(&w[(size_t)j * H * H], b.w(fmt("sy.enc.l%d.", l) + nm[j] + ".w"), (size_t)H * H * 4);
            memcpy(&bb[(size_t)j * H], b.w(fmt("sy.enc.l%d.", l) + nm[j] + ".b"), (size_t)H * 4);
        }
        L.qkv = prep_conv(w.data(), bb.data(), 3 * H, H, 1, 1);
        L.o = prep_conv(b.w(fmt("sy.enc.l%d.o.w", l)), b.w(fmt("sy.enc.l%d.o.b", l)), H, H, 1, 1);
        L.ff1 = prep_conv(b.w(fmt("sy.enc.l%d.ff1.w", l)), b.w(fmt("sy.enc.l%d.ff1.b", l)), filter, H, enc_k, 1);
        L.ff2 = prep_conv(b.w(fmt("sy.enc.l%d.ff2.w", l)), b.w(fmt("sy.enc.l%d.ff2.b", l)), H, filter, enc_k, 1);
        L.rel_k = own(fmt("sy.enc.l%d.rel_k", l)); L.rel_v = own(fmt("sy.enc.l%d.rel_v", l));
        L.ln1_g = own(fmt("sy.enc.l%d.ln1.g", l)); L.ln1_b = own(fmt("sy.enc.l%d.ln1.b", l));
        L.ln2_g = own(fmt("sy.enc.l%d.ln2.g", l)); L.ln2_b = own(fmt("sy.enc.l%d.ln2.b", l));
        if (H >= 128 && H % 16 == 0 && !test_opt("RVC_NO_LN_FUSE")) {
            has_folded = true;
            if (l > 0) L.qkv_f = ModelCV::fold_ln(w.data(), bb.data(), 3 * H, H, b.w(fmt("sy.enc.l%d.ln2.g", l - 1)), b.w(fmt("sy.enc.l%d.ln2.b", l - 1)), &L.qkv_wsum);
        }
        layers.push_back(L);
    }
    proj = prep_conv(b.w("sy.enc.proj.w"), b.w("sy.enc.proj.b"), 2 * inter, H, 1, 1);
    if (has_folded)
        proj_f = ModelCV::fold_ln(b.w("sy.enc.proj.w"), b.w("sy.enc.proj.b"), 2 * inter, H, b.w(fmt("sy.enc.l%d.ln2.g", enc_layers - 1)), b.w(fmt("sy.enc.l%d.ln2.b", enc_layers - 1)), &proj_wsum);
    const int half = inter / 2;
    for (int i = 0; i < flow_n; i++) {
        Flow F;
        // Flip layers are folded into the weights: the latent stays in its physical channel order and a flow that sees it
        // flipped (inference runs flip -> coupling from the last flow to the first: flow i after flow_n - i flips) reads its
        // x0 from the upper half with reversed input columns and writes x1 to the lower half with reversed output rows
        F.flipped = ((flow_n - i) & 1) != 0;
        {
            // rows H..2H are zero: the launch also clears the skip accumulator that sits behind hh in one tensor
            std::vector<float> w((size_t)2 * H * half, 0.f), bb((size_t)2 * H, 0.f);
            const float *pw = b.w(fmt("sy.flow%d.pre.w", i)), *pb = b.w(fmt("sy.flow%d.pre.b", i));
            for (int r = 0; r < H; r++) {
                bb[r] = pb[r];
                for (int q = 0; q < half; q++) w[(size_t)r * half + q] = pw[(size_t)r * half + (F.flipped ? half - 1 - q : q)];
            }
            F.pre = prep_conv(w.data(), bb.data(), 2 * H, half, 1, 1);
            F.h_pre_w.assign(w.begin(), w.begin() + (size_t)H * half); F.h_pre_b.assign(bb.begin(), bb.begin() + H);
        }
        // speaker conditioning is a constant of the chunk (sid baked, rvc.rs:186-187): fold cond(g) into the in-layer biases.  This host fold of sy.g
        // is what holds after load; a blob with a speaker table can refold the same buffers on the device (speaker.hip.h, speaker_setup below)
        const float *cw = b.w(fmt("sy.flow%d.cond.w", i)), *cb = b.w(fmt("sy.flow%d.cond.b", i));
        for (int j = 0; j < wn_layers; j++) {
            std::vector<float> bias(2 * H);
            const float *ib = b.w(fmt("sy.flow%d.in%d.b", i, j));
            for (int r = 0; r < 2 * H; r++) {
                float a = cb[j * 2 * H + r];
                for (int q = 0; q < G; q++) a += cw[(size_t)(j * 2 * H + r) * G + q] * g[q];
                bias[r] = ib[r] + a;
            }
            {
                const float *iw = b.w(fmt("sy.flow%d.in%d.w", i, j));
                const size_t Kin = (size_t)H * wn_k;
                std::vector<float> w, pb;
                glu_pack_rows(iw, bias.data(), H, Kin, w, pb);
                F.in.push_back(prep_conv(w.data(), pb.data(), 2 * H, H, wn_k, 1));
                F.h_in_w.emplace_back(iw, iw + (size_t)2 * H * Kin); F.h_in_b.push_back(bias);
            }
            int rs_c = j < wn_layers - 1 ? 2 * H : H;
            F.rs.push_back(prep_conv(b.w(fmt("sy.flow%d.rs%d.w", i, j)), b.w(fmt("sy.flow%d.rs%d.b", i, j)), rs_c, H, 1, 1));
            { const float *rw = b.w(fmt("sy.flow%d.rs%d.w", i, j)), *rb = b.w(fmt("sy.flow%d.rs%d.b", i, j)); F.h_rs_w.emplace_back(rw, rw + (size_t)rs_c * H); F.h_rs_b.emplace_back(rb, rb + rs_c); }
        }
        {
            const float *pw = b.w(fmt("sy.flow%d.post.w", i)), *pb = b.w(fmt("sy.flow%d.post.b", i));
            std::vector<float> w((size_t)half * H), bb(half);
            for (int r = 0; r < half; r++) {
                const int src = F.flipped ? half - 1 - r : r;
                memcpy(&w[(size_t)r * H], pw + (size_t)src * H, (size_t)H * sizeof(float));
                bb[r] = pb[src];
            }
            F.post = prep_conv(w.data(), bb.data(), half, H, 1, 1);
            F.h_post_w = w; F.h_post_b = bb;
        }
        flows.push_back(F);
    }
    // composed WaveNets (one to eight streams): built with the model, 20 tasks on the host's cores, so that no first chunk pays for them
    if (hidden % 16 == 0 && inter == hidden && !test_opt("RVC_NO_WN_COMPOSE")) compose_flows();
    {
        std::vector<float> bias(up_init);
        const float *cw = b.w("sy.dec.cond.w"), *cb = b.w("sy.dec.cond.b"), *pb = b.w("sy.dec.pre.b");
        for (int c = 0; c < up_init; c++) { float a = cb[c]; for (int q = 0; q < G; q++) a += cw[(size_t)c * G + q] * g[q]; bias[c] = pb[c] + a; }
        dec_pre = prep_conv(b.w("sy.dec.pre.w"), bias.data(), up_init, inter, 7, 1);
    }
    int c = up_init;
    for (int i = 0; i < n_ups; i++) {
        int co = c / 2;
        ups.push_back(prep_convT1d(b.w(fmt("sy.dec.up%d.w", i)), b.w(fmt("sy.dec.up%d.b", i)), c, co, up_kernel[i], up_rate[i]));
        int sf = 1; for (int q = i + 1; q < n_ups; q++) sf *= up_rate[q];
        int nk = i + 1 < n_ups ? 2 * sf : 1;
        if (has_f0) ncs.push_back(prep_conv(b.w(fmt("sy.dec.nc%d.w", i)), b.w(fmt("sy.dec.nc%d.b", i)), co, 1, nk, 1));
        std::vector<std::vector<std::pair<ConvW, ConvW>>> stage;
        for (int j = 0; j < n_rb; j++) {
            std::vector<std::pair<ConvW, ConvW>> chain;
            for (int m = 0; m < n_rbd; m++) {
                ConvW c1 = prep_conv(b.w(fmt("sy.dec.rb%d_%d.c1_%d.w", i, j, m)), b.w(fmt("sy.dec.rb%d_%d.c1_%d.b", i, j, m)), co, co, rb_k[j], 1);
                ConvW c2 = prep_conv(b.w(fmt("sy.dec.rb%d_%d.c2_%d.w", i, j, m)), b.w(fmt("sy.dec.rb%d_%d.c2_%d.b", i, j, m)), co, co, rb_k[j], 1);
                chain.push_back({c1, c2});
            }
            stage.push_back(chain);
        }
        rbs.push_back(stage);
        // the n_rb chains' q-th convs run as phases of one launch: their weights share an allocation
        for (int m = 0; m < n_rbd && n_rb > 1; m++) {
            std::vector<ConvW *> a, bb;
            for (int j = 0; j < n_rb; j++) { a.push_back(&rbs.back()[j][m].first); bb.push_back(&rbs.back()[j][m].second); }
            merge_convs(a); merge_convs(bb);
        }
        c = co;
    }
    dec_post = prep_conv(b.w("sy.dec.post.w"), nullptr, 1, c, 7, 1);
    if (has_f0) { src_w = b.w("sy.src")[0]; src_b = b.w("sy.src")[1]; }
    weight_bytes = b.bytes();
    // the f0 / feature frame rate is 100 Hz (rvc.rs:153, 160 samples @16 kHz): a synthesizer whose hop is not sr / 100 would
    // return audio of the wrong length without any error (e.g. an import that guessed the first upsample rate)
    if (sr != 100 * upp()) throw std::runtime_error(fmt("synthesizer: sr %d", sr) + fmt(" != 100 * prod(upsample rates) = %d", 100 * upp()));
    n_spk = b.icfg_or("n_spk", 1);
    if (b.has("sy.emb_g")) speaker_setup(b);
    else if (n_spk != 1) throw std::runtime_error(fmt("synthesizer: n_spk = %d without a speaker table (sy.emb_g)", n_spk));
}

// ------------------------------- run-time speaker selection (speaker.hip.h) ------------------------------------------
// A blob with a speaker table: the table, every cond layer and the unfolded biases go to the device (about 5 MB at full size), and the table of the
// conditioned layers is built: flow 0 layer 0, flow 0 layer 1, ..., dec_pre -- the order of rvc_debug_speaker_biases.  The biases themselves stay the
// host fold of sy.g until a set call.
void ModelSY::speaker_setup(const Blob &b)
{
    const BlobTensor &tb = b.t("sy.emb_g");
    if (tb.dims.size() != 2 || tb.dims[0] != n_spk || tb.dims[1] != gin || n_spk < 1) throw std::runtime_error("synthesizer: sy.emb_g is not [n_spk][gin]");
    const float *g = b.w("sy.g");
    sid_g = -1;
    for (int i = 0; i < n_spk && sid_g < 0; i++) if (memcmp(tb.data + (size_t)i * gin, g, (size_t)gin * sizeof(float)) == 0) sid_g = i;
    if (sid_g < 0) throw std::runtime_error("synthesizer: sy.g is no row of the speaker table sy.emb_g");
    mix_n = 1; mix_id[0] = sid_g; mix_w[0] = 1.0;
    auto own = [&](const std::string &n) { float *p = dv(b, n); owned.push_back(p); return p; };
    spk_emb = own("sy.emb_g");
    const int H = hidden;
    int row0 = 0;
    for (int i = 0; i < flow_n; i++) {
        const float *cw = own(fmt("sy.flow%d.cond.w", i)), *cb = own(fmt("sy.flow%d.cond.b", i));
        for (int j = 0; j < wn_layers; j++) {
            SpeakerLayer L{};
            L.base_b = own(fmt("sy.flow%d.in%d.b", i, j)); L.cond_w = cw + (size_t)j * 2 * H * gin; L.cond_b = cb + (size_t)j * 2 * H;
            L.row0 = row0; L.rows = 2 * H; L.glu_h = H;
            spk_layers.push_back(L); row0 += L.rows;
        }
    }
    {
        SpeakerLayer L{};
        L.base_b = own("sy.dec.pre.b"); L.cond_w = own("sy.dec.cond.w"); L.cond_b = own("sy.dec.cond.b");
        L.row0 = row0; L.rows = up_init; L.glu_h = 0;
        spk_layers.push_back(L); row0 += L.rows;
    }
    spk_rows = row0;
    HIPCHK(hipMalloc(&d_spk_layers, spk_layers.size() * sizeof(SpeakerLayer)));
    HIPCHK(hipMalloc(&d_spk_mix, sizeof(SpeakerMix)));
    HIPCHK(hipHostMalloc(&h_spk_mix, 8 * sizeof(SpeakerMix)));
    speaker_targets();
}
// where the fold stores: the live bias buffers as they are now (the composed twins exist only once compose_flows has run).  Called at load and behind every
// compose_flows; a compose that comes late has built its biases from the host fold of sy.g, so a mix that a set call has put in force is folded again
void ModelSY::speaker_targets()
{
    if (!d_spk_layers) return;
    HIPCHK(hipDeviceSynchronize());      // a queued fold may still be reading the table
    size_t k = 0;
    for (int i = 0; i < flow_n; i++)
        for (int j = 0; j < wn_layers; j++, k++) { spk_layers[k].dst0 = flows[i].in[j].bias; spk_layers[k].dst1 = composed ? flows[i].inc[j].bias : nullptr; }
    spk_layers[k].dst0 = dec_pre.bias; spk_layers[k].dst1 = nullptr;
    HIPCHK(hipMemcpy(d_spk_layers, spk_layers.data(), spk_layers.size() * sizeof(SpeakerLayer), hipMemcpyHostToDevice));
    if (!spk_baked) spk_dirty = true;
}
// the mix by ids and weights: n in [1, 8], ids in [0, n_spk) and distinct, weights finite, >= 0 and not all zero; normalised to sum 1 in double.  A model
// without a table has the one speaker 0 (sy.g): {0: w} is accepted and changes nothing
void ModelSY::set_speaker_mix(const int32_t *sid, const double *weight, size_t n)
{
    if (n < 1 || n > (size_t)SPK_MAX_MIX || !sid || !weight) throw ShapeError("speaker mix: 1 to 8 (id, weight) pairs");
    double sum = 0.0;
    for (size_t i = 0; i < n; i++) {
        if (sid[i] < 0 || sid[i] >= n_spk) throw ShapeError(fmt("speaker mix: id %d outside [0, %d)", (int)sid[i], n_spk));
        for (size_t k = 0; k < i; k++) if (sid[k] == sid[i]) throw ShapeError(fmt("speaker mix: id %d repeated", (int)sid[i]));
        if (!std::isfinite(weight[i]) || weight[i] < 0.0) throw ShapeError("speaker mix: a weight is negative or not finite");
        sum += weight[i];
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) throw ShapeError("speaker mix: the weights sum to 0 (or overflow)");
    if (!has_speaker_table()) return;
    double w[SPK_MAX_MIX];
    for (size_t i = 0; i < n; i++) w[i] = weight[i] / sum;
    bool same = !spk_baked && (size_t)mix_n == n;
    for (size_t i = 0; i < n && same; i++) same = mix_id[i] == sid[i] && mix_w[i] == w[i];
    if (same) return;
    mix_n = (int)n;
    for (size_t i = 0; i < n; i++) { mix_id[i] = sid[i]; mix_w[i] = w[i]; }
    spk_baked = false; spk_dirty = true;
}
void ModelSY::queue_speaker_fold(hipStream_t s, bool profile)
{
    if (!spk_dirty || !has_speaker_table()) return;
    // every fold writes its own pinned block; a block is rewritten only after the copy that last read it has completed
    const unsigned us = spk_slot++ & 7u;
    if (spk_ev_used[us]) HIPCHK(hipEventSynchronize(spk_ev[us]));
    SpeakerMix *h = h_spk_mix + us;
    memset(h, 0, sizeof *h);
    h->n = mix_n;
    for (int i = 0; i < mix_n; i++) { h->id[i] = mix_id[i]; h->w[i] = (float)mix_w[i]; }
    HIPCHK(hipMemcpyAsync(d_spk_mix, h, sizeof(SpeakerMix), hipMemcpyHostToDevice, s));
    if (!spk_ev[us]) HIPCHK(hipEventCreateWithFlags(&spk_ev[us], hipEventDisableTiming));
    HIPCHK(hipEventRecord(spk_ev[us], s)); spk_ev_used[us] = true;
    if (profile) { for (auto &ev : spk_prof) if (!ev) HIPCHK(hipEventCreate(&ev)); HIPCHK(hipEventRecord(spk_prof[0], s)); }
    const int wgs = std::min((spk_rows + SPK_WAVES - 1) / SPK_WAVES, SPK_MAX_WGS);
    hipLaunchKernelGGL(speaker_fold_kernel, dim3(wgs), dim3(SPK_WAVES * 64), (size_t)(gin + 3) / 4 * 16, s, d_spk_mix, spk_emb, n_spk, gin, d_spk_layers, (int)spk_layers.size(), spk_rows);
    if (profile) { HIPCHK(hipEventRecord(spk_prof[1], s)); spk_prof_valid = true; }
    spk_dirty = false;
}
// the live biases of every conditioned layer in model row order (the in-layers un-packed), of the plain copies or of the composed twins (+ dec_pre either way)
void ModelSY::speaker_biases(bool composed_copy, std::vector<float> &out)
{
    if (composed_copy && !composed) throw ShapeError("speaker biases: the flows are not composed");
    HIPCHK(hipDeviceSynchronize());
    const int H = hidden;
    out.clear();
    std::vector<float> pk((size_t)std::max(2 * H, up_init));
    for (int i = 0; i < flow_n; i++)
        for (int j = 0; j < wn_layers; j++) {
            HIPCHK(hipMemcpy(pk.data(), composed_copy ? flows[i].inc[j].bias : flows[i].in[j].bias, (size_t)2 * H * sizeof(float), hipMemcpyDeviceToHost));
            for (int m = 0; m < 2 * H; m++) out.push_back(pk[glu_packed_row(m, H)]);
        }
    HIPCHK(hipMemcpy(pk.data(), dec_pre.bias, (size_t)up_init * sizeof(float), hipMemcpyDeviceToHost));
    out.insert(out.end(), pk.begin(), pk.begin() + up_init);
}
// One stream: every flow's WaveNet runs 4 x (gated k-tap in-layer, 1x1 res_skip layer) -- ten dependent launches of a 21-column window.  The
// res_skip layers are linear, so they are composed into what follows them (exactly, in double, when the model is loaded):
//   x_j = h0 + sum_{i<j} (R_i a_i + r_i)                      =>  in_j(x_j) = W_j * [1 | h0 | a_0 .. a_{j-1}]   with W_j(a_i) = W_j o R_i
//   post(skip) = P (sum_j S_j a_j + s_j) + p                   =>  one 1x1 layer over [a_0 .. a_{n-1}]
// (R_i / S_i: the residual / skip rows of res_skip layer i; the constant r_i rides on a row of ones -- zero in the halo, like the zero padding
// the in-layer sees -- so the edges of the window stay exact.)  The latent z rides in the same tensor ([ones | h0 | a_0 .. | z]), and a flow's
// post layer and the NEXT flow's pre layer become one 1x1 layer over [a_0 .. a_{n-1} | z] that writes h0_next and z_next into the other of two
// such tensors (two phases of one launch: same input, two outputs): five launches per flow (+ one pre at the start) instead of ten.
void ModelSY::compose_flows()
{
    if (composed) return;
    const int H = hidden, I = inter, half = inter / 2, K5 = wn_k, nl = wn_layers;
    const int nfl = (int)flows.size();
    // per flow: x0 / x1 rows of the latent, the full-latent pre weights [H][I] (zero on the x1 half), post rows on the x1 half
    auto x1_row0 = [&](const Flow &F) { return F.flipped ? 0 : half; };
    auto x0_row0 = [&](const Flow &F) { return F.flipped ? half : 0; };
    std::vector<std::vector<std::vector<float>>> WJ(nfl), BJ(nfl);
    std::vector<std::vector<float>> WM(nfl), BM(nfl), WH(nfl), BH(nfl), WP1(nfl), BP1(nfl);
    // in-layer j of flow fi over [ones16 | h0 | a_0 .. a_{j-1}] (one task each: 1.7 GFLOP of double arithmetic in all, spread over the host's cores)
    auto in_layer = [&](int fi, int j) {
        Flow &F = flows[fi];
        {
            const int Cin = 16 + H * (j + 1), a0 = 16 + H;
            std::vector<double> w((size_t)2 * H * Cin * K5, 0.0);
            const float *W5 = F.h_in_w[j].data();                 // [2H][H][K5], model row order
            for (int o = 0; o < 2 * H; o++)
                for (int mm = 0; mm < H; mm++)
                    for (int t = 0; t < K5; t++) w[((size_t)o * Cin + 16 + mm) * K5 + t] = W5[((size_t)o * H + mm) * K5 + t];
            std::vector<double> acc(H);
            for (int i = 0; i < j; i++) {
                const float *Rr = F.h_rs_w[i].data(), *rb = F.h_rs_b[i].data();      // rows 0..H: the residual part
                for (int o = 0; o < 2 * H; o++)
                    for (int t = 0; t < K5; t++) {
                        std::fill(acc.begin(), acc.end(), 0.0);
                        double one = 0.0;
                        for (int mm = 0; mm < H; mm++) {
                            const double v = W5[((size_t)o * H + mm) * K5 + t];
                            const float *Rm = Rr + (size_t)mm * H;
                            for (int c = 0; c < H; c++) acc[c] += v * Rm[c];
                            one += v * rb[mm];
                        }
                        for (int c = 0; c < H; c++) w[((size_t)o * Cin + a0 + H * i + c) * K5 + t] = acc[c];
                        w[((size_t)o * Cin) * K5 + t] += one;
                    }
            }
            std::vector<float> wp, pb;
            glu_pack_rows(w.data(), F.h_in_b[j].data(), H, (size_t)Cin * K5, wp, pb);      // as for the plain in-layers
            WJ[fi][j] = std::move(wp); BJ[fi][j] = std::move(pb);
        }
    };
    auto one_flow = [&](int fi) {
        Flow &F = flows[fi];
        // first launch of the flow when it has no predecessor in processing order: h0 = pre(x0) from the full latent
        WP1[fi].assign((size_t)H * I, 0.f); BP1[fi] = F.h_pre_b;
        for (int r = 0; r < H; r++) for (int q = 0; q < half; q++) WP1[fi][(size_t)r * I + x0_row0(F) + q] = F.h_pre_w[(size_t)r * half + q];
        // composed post over [a_0 .. a_{n-1}]: P (sum_j S_j a_j + s_j) + p, rows = the x1 half in its physical order
        const int KA = nl * H, Kin = KA + I;                       // last launch's input: [a_0 .. a_{n-1} | z]
        std::vector<double> pc((size_t)half * KA, 0.0), pcb(half, 0.0);
        for (int r = 0; r < half; r++) {
            double bacc = F.h_post_b[r];
            for (int j = 0; j < nl; j++) {
                const int row0 = j < nl - 1 ? H : 0;               // skip rows of res_skip layer j
                const float *S = F.h_rs_w[j].data() + (size_t)row0 * H, *sb = F.h_rs_b[j].data() + row0;
                for (int h = 0; h < H; h++) {
                    const double v = F.h_post_w[(size_t)r * H + h];
                    for (int c = 0; c < H; c++) pc[(size_t)r * KA + (size_t)j * H + c] += v * S[(size_t)h * H + c];
                    bacc += v * sb[h];
                }
            }
            pcb[r] = bacc;
        }
        // last launch of the flow, input [A | z] (K = n H + I): z_next = z - [0 ; post(A)] on the x1 rows, and for the next flow in processing order
        //   h0_next = pre_next(z_next) = Wn z - Wn[:, x1 rows] post(A) + (bn - Wn[:, x1 rows] p)        (two phases of one launch: same input, two outputs)
        const bool has_next = fi > 0;
        const int r1 = x1_row0(F);
        std::vector<double> wz((size_t)I * Kin, 0.0), bz(I, 0.0);
        for (int c = 0; c < I; c++) wz[(size_t)c * Kin + KA + c] = 1.0;
        for (int r = 0; r < half; r++) {
            for (int q = 0; q < KA; q++) wz[(size_t)(r1 + r) * Kin + q] = -pc[(size_t)r * KA + q];
            bz[r1 + r] = -pcb[r];
        }
        WM[fi].resize(wz.size()); BM[fi].resize(I);
        for (size_t q = 0; q < wz.size(); q++) WM[fi][q] = (float)wz[q];
        for (int r = 0; r < I; r++) BM[fi][r] = (float)bz[r];
        if (has_next) {
            const Flow &N = flows[fi - 1];
            std::vector<double> wh((size_t)H * Kin, 0.0);
            WH[fi].resize(wh.size()); BH[fi].resize(H);
            for (int r = 0; r < H; r++) {
                double bacc = N.h_pre_b[r];
                for (int q = 0; q < half; q++) {
                    const double v = N.h_pre_w[(size_t)r * half + q];
                    const int zc = x0_row0(N) + q;                 // latent row this weight multiplies
                    wh[(size_t)r * Kin + KA + zc] += v;
                    if (zc >= r1 && zc < r1 + half) {
                        const int pr = zc - r1;
                        for (int c = 0; c < KA; c++) wh[(size_t)r * Kin + c] -= v * pc[(size_t)pr * KA + c];
                        bacc -= v * pcb[pr];
                    }
                }
                BH[fi][r] = (float)bacc;
            }
            for (size_t q = 0; q < wh.size(); q++) WH[fi][q] = (float)wh[q];
        }
    };
    for (int i = 0; i < nfl; i++) { WJ[i].resize(nl); BJ[i].resize(nl); }
    std::vector<std::thread> th;
    for (int i = 0; i < nfl; i++) {
        th.emplace_back([&, i]() { one_flow(i); });
        for (int j = 0; j < nl; j++) th.emplace_back([&, i, j]() { in_layer(i, j); });
    }
    for (auto &t : th) t.join();
    for (int i = 0; i < nfl; i++) {
        Flow &F = flows[i];
        F.pre1 = prep_conv(WP1[i].data(), BP1[i].data(), H, I, 1, 1);
        for (int j = 0; j < nl; j++) F.inc.push_back(prep_conv(WJ[i][j].data(), BJ[i][j].data(), 2 * H, 16 + H * (j + 1), K5, 1));
        F.postc = prep_conv(WM[i].data(), BM[i].data(), I, nl * H + I, 1, 1);
        if (i > 0) {
            F.posth = prep_conv(WH[i].data(), BH[i].data(), H, nl * H + I, 1, 1);
            std::vector<float> pb(BH[i]); pb.insert(pb.end(), BM[i].begin(), BM[i].end());
            F.pair_bias = upload_f(pb); owned.push_back(F.pair_bias);
        }
    }
    composed = true;
    speaker_targets();
}
ModelSY::~ModelSY()
{
    free_conv(phone); free_conv(proj); free_conv(dec_pre); free_conv(dec_post);
    for (auto &L : layers) { free_conv(L.qkv); free_conv(L.o); free_conv(L.ff1); free_conv(L.ff2); free_conv(L.qkv_f); if (L.qkv_wsum) wfree(L.qkv_wsum); }
    free_conv(proj_f); if (proj_wsum) wfree(proj_wsum);
    for (auto &F : flows) { free_conv(F.pre); free_conv(F.post); for (auto &c : F.in) free_conv(c); for (auto &c : F.rs) free_conv(c); if (composed) { free_conv(F.pre1); free_conv(F.postc); free_conv(F.posth); for (auto &c : F.inc) free_conv(c); } }
    for (auto &c : ups) free_conv(c);
    for (auto &c : ncs) free_conv(c);
    for (auto &s : rbs) for (auto &ch : s) for (auto &pr : ch) { free_conv(pr.first); free_conv(pr.second); }
    for (float *p : owned) wfree(p);
    if (d_spk_layers) (void)hipFree(d_spk_layers);
    if (d_spk_mix) (void)hipFree(d_spk_mix);
    if (h_spk_mix) (void)hipHostFree(h_spk_mix);
    for (auto &ev : spk_ev) if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : spk_prof) if (ev) (void)hipEventDestroy(ev);
}

// ------------------------------- synthesizer ------------------------------------------
// NSF harmonic source (SineGen + Linear(1, 1) + tanh) of pitchf [B][R] into src [B][1][R upp]; the noise is drawn per stream from st / cp (stream_id, chunk, seed);
// the source reads f0 x f0_num / f0_den.  The kernel keeps the per-frame phases of one stream in 512-entry tables: longer windows are refused.
void add_nsf_source(Plan &pl, int B, const float *pitchf, const T1 &src, int R, int upp, float sr, float lin_w, float lin_b, const StreamState *st, const CallParams *cp,
                    int f0_num, int f0_den)
{
    if (R > 512) throw ShapeError("return_length too long for the NSF source kernel");
    if (R < 1 || upp < 1 || src.T != R * upp || src.C != 1 || f0_den < 1) throw ShapeError("NSF source: inconsistent shapes");
    SrcP sp{}; sp.pitchf = pitchf; sp.src = src.p; sp.src_bs = src.bs; sp.T = R; sp.upp = upp; sp.sr = sr;
    sp.lin_w = lin_w; sp.lin_b = lin_b; sp.st = st; sp.cp = cp;
    sp.f0_num = f0_num; sp.f0_den = f0_den;
    pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(nsf_source_kernel, dim3(B), dim3(1024), 0, s, sp); });
}

// The source depends only on the f0 branch, so it is queued on that branch's stream
T1 build_nsf_source(rvc_engine *e, Plan &pl, int B, float *d_pitchf)
{
    ModelSY &m = *e->sy;
    if (!m.has_f0) throw std::logic_error("NSF source on a model without pitch guidance");
    Arena &A = pl.arena;
    const int R = (int)pl.key.R, R2 = pl.dec_frames();
    const int upp = m.upp();
    const size_t N = (size_t)R * upp;
    if (R > 512) throw ShapeError("return_length too long for the NSF source kernel");
    int max_sf = 1; { int sf = 1; for (int i = m.n_ups - 1; i >= 1; i--) { sf *= m.up_rate[i]; max_sf = std::max(max_sf, sf); } }
    T1 src = make_t1(A, B, 1, (int)N, max_sf + 2);
    add_nsf_source(pl, B, d_pitchf, src, R, upp, (float)m.sr, m.src_w, m.src_b, e->d_state, e->d_cp, R2, R);        // formant shift: f0 x R2 / R compensates the time stretch below (1 without one)
    add_tap(pl, "sy.src", src);
    if (!pl.key.fstage) return src;
    // formant shift: the source stretched to R2 frames (formant.hip.h)
    T1 srci = src;
    if (R2 != R) {
        srci = make_t1(A, B, 1, R2 * upp, max_sf + 2);
        const int Nin = (int)N, Nout = R2 * upp; dim3 grid((Nout + 255) / 256, B);
        pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(time_lerp_kernel, grid, dim3(256), 0, s, src.p, src.ld, src.bs, srci.p, srci.ld, srci.bs, 1, Nin, Nout); });
    }
    add_tap(pl, "sy.srci", srci);
    return srci;
}

// The decoder adds a strided convolution of the harmonic source to the output of every upsampling stage.  Those convolutions depend on
// the source only: they are queued right behind it on the side stream (next to the text encoder and the flow) and the upsampling
// convolution takes their result as its residual -- 4 launches off the serial chain; the sum has the same operands as before.
std::vector<T1> build_noise_convs(rvc_engine *e, Plan &pl, int B, const T1 &src)
{
    ModelSY &m = *e->sy;
    if (!m.has_f0) throw std::logic_error("noise convolutions on a model without pitch guidance");
    std::vector<T1> nz;
    int c = m.up_init, Tc = pl.dec_frames();
    for (int i = 0; i < m.n_ups; i++) {
        const int co = c / 2, Tn = Tc * m.up_rate[i];
        T1 t = make_t1(pl.arena, B, co, Tn, 0);
        int sf = 1; for (int q = i + 1; q < m.n_ups; q++) sf *= m.up_rate[q];
        if (i + 1 < m.n_ups) add_conv1d(pl, m.ncs[i], src, t, sf, sf / 2, 1); else add_conv1d(pl, m.ncs[i], src, t, 1, 0, 1);
        nz.push_back(t);
        c = co; Tc = Tn;
    }
    return nz;
}

void build_synth(rvc_engine *e, Plan &pl, int B, const T1 &phone, const T1 &src, float *d_pitchf, int *d_pitch, int src_join_sid,
                        const std::vector<T1> *nz)
{
    ModelSY &m = *e->sy;
    Arena &A = pl.arena;
    const int R = (int)pl.key.R, H = m.hidden, I = m.inter, F = m.filter, half = I / 2;
    const int HALO = 4;
    if (m.enc_k / 2 > HALO || m.wn_k / 2 > HALO) throw ShapeError("synth kernel sizes exceed the halo");
    T1 z = make_t1(A, B, I, R, HALO), zf = make_t1(A, B, I, R, HALO);
    {
        T1 x = make_t1(A, B, H, R, HALO);
        add_conv1d(pl, m.phone, phone, x, 1, 0, 1);
        {
            dim3 grid((H * R + 255) / 256, B); float *emb = m.pitch_emb; float sq = sqrtf((float)H);
            if (m.has_f0) pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(embed_pitch_kernel, grid, dim3(256), 0, s, x.p, x.ld, x.bs, emb, d_pitch, H, R, sq); });
            else pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(embed_nopitch_kernel, grid, dim3(256), 0, s, x.p, x.ld, x.bs, H, R, sq); });
        }
        add_tap(pl, "sy.emb", x);
        T1 qkv = make_t1(A, B, 3 * H, R, 0), att = make_t1(A, B, H, R, 0), ff = make_t1(A, B, F, R, HALO);
        // one stream: the second LayerNorm of every encoder layer is folded into the next projection (see build_contentvec)
        const bool fuse_ln = B <= LN_FOLD_MAX_STREAMS && m.has_folded && !pl.key.plain_plan && !test_opt("RVC_NO_LN_FUSE");
        bool raw = false; const float *raw_g = nullptr, *raw_b = nullptr; float *raw_st = nullptr;
        for (int l = 0; l < m.enc_layers; l++) {
            ModelSY::Layer &Ly = m.layers[l];
            if (raw) { raw_st = A.floats((size_t)2 * R + 16); ConvOpts o; o.ln_wsum = Ly.qkv_wsum; o.ln_stats_out = raw_st; o.ln_rows = H; add_conv1d(pl, Ly.qkv_f, x, qkv, 1, 0, 1, o); }
            else add_conv1d(pl, Ly.qkv, x, qkv, 1, 0, 1);
            add_relpos_attention(pl, qkv, att, m.heads, Ly.rel_k, Ly.rel_v, m.window);
            {
                ConvOpts o; o.res = x.p; o.res_cs = x.ld; o.res_bs = x.bs;
                if (raw) { o.ln_stats_in = raw_st; o.ln_g = raw_g; o.ln_b = raw_b; }
                add_conv1d(pl, Ly.o, att, x, 1, 0, 1, o);
            }
            add_layernorm(pl, x, Ly.ln1_g, Ly.ln1_b);
            { ConvOpts o; o.act = ACT_RELU; add_conv1d(pl, Ly.ff1, x, ff, 1, m.enc_k / 2, 1, o); }
            { ConvOpts o; o.res = x.p; o.res_cs = x.ld; o.res_bs = x.bs; add_conv1d(pl, Ly.ff2, ff, x, 1, m.enc_k / 2, 1, o); }
            if (fuse_ln) { raw = true; raw_g = Ly.ln2_g; raw_b = Ly.ln2_b; }
            else add_layernorm(pl, x, Ly.ln2_g, Ly.ln2_b);
        }
        add_tap(pl, raw ? "sy.enc.raw" : "sy.enc", x);
        // one stream: WaveNets with their res_skip layers composed away and post + next pre merged (ModelSY::compose_flows): 21 launches for
        // four flows instead of 40.  U[k] = [ones16 | h0 (H) | a_0 .. a_{n-1} | z (I)]; flow k reads U[k & 1] and writes h0 and z of U[(k + 1) & 1]
        static const int wn_max_b = tune_env("RVC_WN_COMPOSE_MAX") ? atoi(tune_env("RVC_WN_COMPOSE_MAX")) : 8;
        const bool wn_composed = B <= wn_max_b && H % 16 == 0 && I == H && !pl.key.plain_plan && !test_opt("RVC_NO_WN_COMPOSE");      // (launch-bound up to a few streams)
        T1 U[2];
        const int u_z = 16 + H + H * m.wn_layers;                     // first latent row of U
        if (wn_composed) {
            m.compose_flows();
            std::vector<float> ones(R, 1.0f);
            for (int k = 0; k < 2; k++) {
                U[k] = make_t1(A, B, u_z + I, R, HALO);
                for (int bb = 0; bb < B; bb++) HIPCHK(hipMemcpy(U[k].p + (long long)bb * U[k].bs, ones.data(), (size_t)R * sizeof(float), hipMemcpyHostToDevice));
            }
            z = U[0].rows(u_z, I);                                     // the prior sample lands in U[0]'s latent rows
        }
        T1 stats = make_t1(A, B, 2 * I, R, 0);
        if (raw) { ConvOpts o; o.ln_wsum = m.proj_wsum; o.ln_rows = H; add_conv1d(pl, m.proj_f, x, stats, 1, 0, 1, o); }
        else add_conv1d(pl, m.proj, x, stats, 1, 0, 1);
        add_tap(pl, "sy.stats", stats);
        {
            dim3 grid(((I * R + 3) / 4 + 255) / 256, B); StreamState *st = e->d_state; CallParams *cp = e->d_cp;
            pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(prior_sample_kernel, grid, dim3(256), 0, s, stats.p, stats.ld, stats.bs, z.p, z.ld, z.bs, I, R, st, cp); });
        }
        add_tap(pl, "sy.zp", z);
        // hh (WaveNet state, rows 0..H) and skip (rows H..2H) share one tensor: the res_skip conv updates both in one launch
        T1 hs = make_t1(A, B, 2 * H, R, HALO), acts = make_t1(A, B, H, R, 0);
        T1 hh = hs.rows(0, H), skip = hs.rows(H, H);
        for (int fi = m.flow_n - 1; fi >= 0; fi--) {
            ModelSY::Flow &Fw = m.flows[fi];
            const T1 x0 = Fw.flipped ? z.rows(half, half) : z.rows(0, half), x1 = Fw.flipped ? z.rows(0, half) : z.rows(half, half);
            if (wn_composed) {
                const int k = m.flow_n - 1 - fi;
                const T1 &Uc = U[k & 1], &Un = U[(k + 1) & 1];
                if (k == 0) add_conv1d(pl, Fw.pre1, Uc.rows(u_z, I), Uc.rows(16, H), 1, 0, 1);
                for (int j = 0; j < m.wn_layers; j++) { ConvOpts o; o.glu = true; add_conv1d(pl, Fw.inc[j], Uc.rows(0, 16 + H * (j + 1)), Uc.rows(16 + H * (j + 1), H), 1, (m.wn_k - 1) / 2, 1, o); }
                if (fi > 0) add_conv1d_two(pl, Fw.posth, Fw.postc, Fw.pair_bias, Uc.rows(16 + H, H * m.wn_layers + I), Un.rows(16, H), Un.rows(u_z, I));
                else add_conv1d(pl, Fw.postc, Uc.rows(16 + H, H * m.wn_layers + I), Un.rows(u_z, I), 1, 0, 1);
                if (fi == 0) z = Un.rows(u_z, I);
                if (pl.key.with_taps) { char nm[32]; snprintf(nm, sizeof nm, "sy.flow%d", fi); add_tap(pl, nm, Un.rows(u_z, I)); } else add_stamp(pl, "sy.flow");
                continue;
            }
            add_conv1d(pl, Fw.pre, x0, hs, 1, 0, 1);                       // hh = pre(x0), skip = 0
            for (int j = 0; j < m.wn_layers; j++) {
                { ConvOpts o; o.glu = true; add_conv1d(pl, Fw.in[j], hh, acts, 1, (m.wn_k - 1) / 2, 1, o); }   // acts = tanh(.) * sigmoid(.)
                ConvOpts o; o.accumulate = true;
                if (j < m.wn_layers - 1) add_conv1d(pl, Fw.rs[j], acts, hs, 1, 0, 1, o);     // hh += res, skip += skip part
                else add_conv1d(pl, Fw.rs[j], acts, skip, 1, 0, 1, o);
            }
            { ConvOpts o; o.scale = -1.f; o.accumulate = true; add_conv1d(pl, Fw.post, skip, x1, 1, 0, 1, o); }
            if (pl.key.with_taps) { char nm[32]; snprintf(nm, sizeof nm, "sy.flow%d", fi); add_tap(pl, nm, z); } else add_stamp(pl, "sy.flow");
        }
        if (m.flow_n & 1) {
            // odd number of flips: materialise the last one
            T1 zi = z, zo = zf; dim3 grid((I * R + 255) / 256, B);
            pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(flip_channels_kernel, grid, dim3(256), 0, s, zi.p, zi.ld, zi.bs, zo.p, zo.ld, zo.bs, I, R); });
            std::swap(z, zf);
        }
    }
    add_tap(pl, "sy.z", z);
    const int upp = m.upp();
    const int R2 = pl.dec_frames();
    if (pl.key.fstage) {
        // formant shift: the latent stretched to R2 frames; the decoder runs on them (formant.hip.h)
        if (R2 != R) {
            T1 zi = make_t1(A, B, I, R2, HALO); dim3 grid((I * R2 + 255) / 256, B); T1 zs = z;
            pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(time_lerp_kernel, grid, dim3(256), 0, s, zs.p, zs.ld, zs.bs, zi.p, zi.ld, zi.bs, I, R, R2); });
            z = zi;
        }
        add_tap(pl, "sy.zi", z);
    }
    // decoder
    int max_pad = 3;
    for (int j = 0; j < m.n_rb; j++) for (int q = 0; q < m.n_rbd; q++) max_pad = std::max(max_pad, (m.rb_k[j] * m.rb_d[q] - m.rb_d[q]) / 2);
    const int DH = (max_pad + 3) / 4 * 4;
    int c = m.up_init, Tc = R2;
    if (src_join_sid > 0) pl.ops.join(src_join_sid);     // the harmonic source was produced on a side stream
    T1 xd = make_t1(A, B, c, Tc, DH);
    add_conv1d(pl, m.dec_pre, z, xd, 1, 3, 1);
    add_tap(pl, "sy.pre", xd);
    for (int i = 0; i < m.n_ups; i++) {
        const int co = c / 2, K = m.up_kernel[i], S = m.up_rate[i], Tn = Tc * S;
        if ((K - S) % 2 != 0) throw ShapeError("upsample kernel/stride parity not supported");
        T1 u = make_t1(A, B, co, Tn, DH);
        if (!m.has_f0) {
            // a plain HiFi-GAN generator: no source, nothing to add to the upsampled tensor
            ConvOpts o; o.pre_act = ACT_LRELU; o.pre_slope = 0.1f; add_convT1d(pl, m.ups[i], xd, u, (K - S) / 2, o);
        } else if (nz) {
            const T1 &r = (*nz)[i];
            ConvOpts o; o.pre_act = ACT_LRELU; o.pre_slope = 0.1f; o.res = r.p; o.res_cs = r.ld; o.res_bs = r.bs;
            add_convT1d(pl, m.ups[i], xd, u, (K - S) / 2, o);
        } else {
        { ConvOpts o; o.pre_act = ACT_LRELU; o.pre_slope = 0.1f; add_convT1d(pl, m.ups[i], xd, u, (K - S) / 2, o); }
        int sf = 1; for (int q = i + 1; q < m.n_ups; q++) sf *= m.up_rate[q];
        { ConvOpts o; o.accumulate = true; if (i + 1 < m.n_ups) add_conv1d(pl, m.ncs[i], src, u, sf, sf / 2, 1, o); else add_conv1d(pl, m.ncs[i], src, u, 1, 0, 1, o); }
        }
        if (pl.key.with_taps) { char nm[32]; snprintf(nm, sizeof nm, "sy.up%d", i); add_tap(pl, nm, u); } else add_stamp(pl, "sy.up");
        // the n_rb ResBlock chains of a stage are independent until their average
        T1 xs = make_t1(A, B, co, Tn, DH);
        std::vector<T1> finals;
        const bool fused = m.n_rb > 1 && m.n_rb <= 3 && B < 16 && !tune_env("RVC_SERIAL_RESBLOCKS");   // many streams: every conv fills the chip by itself
        if (fused) {
            // one launch per (dilation, conv): phase j = chain j (kernel size rb_k[j]); 6 launches per stage instead of 6*n_rb
            const int nr = m.n_rb;
            T1 ra = make_t1(A, B, nr * co, Tn, DH), rb = make_t1(A, B, nr * co, Tn, DH), tt = make_t1(A, B, nr * co, Tn, DH), fin = make_t1(A, B, nr * co, Tn, 0);
            T1 cur = u; bool grouped = false;
            for (int q = 0; q < m.n_rbd; q++) {
                const int d = m.rb_d[q];
                std::vector<const ConvW *> c1, c2; std::vector<int> p1, d1, p2, d2;
                for (int j = 0; j < nr; j++) {
                    c1.push_back(&m.rbs[i][j][q].first); c2.push_back(&m.rbs[i][j][q].second);
                    p1.push_back((m.rb_k[j] * d - d) / 2); d1.push_back(d); p2.push_back((m.rb_k[j] - 1) / 2); d2.push_back(1);
                }
                { ConvOpts o; o.pre_act = ACT_LRELU; o.pre_slope = 0.1f; o.act = ACT_LRELU; o.slope = 0.1f; add_conv1d_multi(pl, c1, cur, grouped, tt, p1, d1, o); }
                const bool last = q == m.n_rbd - 1;
                T1 dst = last ? fin : (cur.p == ra.p ? rb : ra);
                ConvOpts o; o.res = cur.p; o.res_cs = cur.ld; o.res_bs = cur.bs;
                add_conv1d_multi(pl, c2, tt, true, dst, p2, d2, o, grouped);
                cur = dst; grouped = true;
            }
            for (int j = 0; j < nr; j++) finals.push_back(fin.rows(j * co, co));
        }
        // Chains issued one after the other (many streams): the average is taken by the chains' last convolutions themselves -- chain j's
        // epilogue stores (j = 0) or adds (j > 0) its output x 1 / n_rb -- instead of three stored tensors and an averaging launch per
        // stage (round 6: 4 launches and ~1 GB of reads + writes per 64-stream step).  The split-bf16 kernels have no accumulating
        // epilogue: those plans keep the averaging launch.
        const bool mean_in_epilogue = !fused && !pl.key.bf3 && test_opt_int("RVC_MEAN3", 0) == 0;     // (test hook RVC_MEAN3 = 1: the averaging launch)
        for (int j = 0; j < m.n_rb && !fused; j++) {
            const int k = m.rb_k[j];
            T1 ra = make_t1(A, B, co, Tn, DH), rb = make_t1(A, B, co, Tn, DH), tt = make_t1(A, B, co, Tn, DH), fin = mean_in_epilogue ? xs : make_t1(A, B, co, Tn, 0);
            T1 cur = u;
            for (int q = 0; q < m.n_rbd; q++) {
                const int d = m.rb_d[q];
                { ConvOpts o; o.pre_act = ACT_LRELU; o.pre_slope = 0.1f; o.act = ACT_LRELU; o.slope = 0.1f; add_conv1d(pl, m.rbs[i][j][q].first, cur, tt, 1, (k * d - d) / 2, d, o); }
                const bool last = q == m.n_rbd - 1;
                T1 dst = last ? fin : (cur.p == ra.p ? rb : ra);
                ConvOpts o; o.res = cur.p; o.res_cs = cur.ld; o.res_bs = cur.bs;
                if (last && mean_in_epilogue) { o.scale = 1.0f / (float)m.n_rb; o.accumulate = j > 0; }
                add_conv1d(pl, m.rbs[i][j][q].second, tt, dst, 1, (k - 1) / 2, 1, o);
                cur = dst;
            }
            finals.push_back(fin);
        }
        if (!mean_in_epilogue) {
            // xs = (r0 + r1 + ...) / n_rb, summed in chain order as in the reference definition
            const int nrb = m.n_rb; const float inv = 1.0f / (float)m.n_rb;
            const float *f0 = finals[0].p, *f1 = nrb > 1 ? finals[1].p : nullptr, *f2 = nrb > 2 ? finals[2].p : nullptr;
            if (nrb > 3) throw ShapeError("more than 3 ResBlock kernels per stage");
            T1 fi = finals[0];
            dim3 grid((co * Tn + 255) / 256, B);
            pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(mean3_kernel, grid, dim3(256), 0, s, f0, f1, f2, fi.ld, fi.bs, xs.p, xs.ld, xs.bs, co, Tn, inv); });
        }
        if (pl.key.with_taps) { char nm[32]; snprintf(nm, sizeof nm, "sy.rb%d", i); add_tap(pl, nm, xs); } else add_stamp(pl, "sy.rb");
        xd = xs; c = co; Tc = Tn;
    }
    if (pl.key.fstage) {
        // formant shift: the decoder's output y2 (R2 upp samples) back to the model rate, R upp samples per stream, by each stream's own
        // descriptor; the kernel writes the caller's buffer when the call provides one (Plan::cur_out)
        T1 dec = make_t1(A, B, 1, Tc, 0);
        { ConvOpts o; o.pre_act = ACT_LRELU; o.pre_slope = 0.01f; o.act = ACT_TANH; o.no_bias = true; add_conv1d(pl, m.dec_post, xd, dec, 1, 3, 1, o); }
        add_tap(pl, "sy.dec", dec);
        const int No = R * upp;
        // (R2 < R for negative shifts: the output is longer than y2; each stream reads y2[0 : R upp_res], checked against R2 upp at upload)
        T1 a; a.p = A.floats((size_t)B * No); a.B = B; a.C = 1; a.T = No; a.ld = No; a.halo = 0; a.bs = No;
        pl.audio = a;
        const Plan *pp = &pl; const StreamState *st = e->d_state; dim3 grid((No + 255) / 256, B);
        pl.ops.push_back([=](hipStream_t s) {
            float *y = pp->cur_out ? pp->cur_out : a.p; const long long ybs = pp->cur_out ? pp->cur_out_bs : (long long)No;
            hipLaunchKernelGGL(formant_resample_kernel, grid, dim3(256), 0, s, dec.p, dec.bs, y, ybs, No, st);
        });
        pl.N = (size_t)No;
        pl.out_direct_ok = !pl.key.with_taps;
        add_stamp(pl, "sy.audio");
        return;
    }
    pl.audio = make_t1(A, B, 1, Tc, 0);
    { ConvOpts o; o.pre_act = ACT_LRELU; o.pre_slope = 0.01f; o.act = ACT_TANH; o.no_bias = true; o.final_out = true; add_conv1d(pl, m.dec_post, xd, pl.audio, 1, 3, 1, o); }
    pl.N = (size_t)Tc;
    pl.out_direct_ok = pl.audio.ld == Tc && !pl.key.with_taps && pl.final_out_honoured;     // (queue_igemm says whether the launch path it chose writes the caller's buffer)
    if (pl.audio.ld != Tc) {
        // make the output rows contiguous [B][N] for the device-pointer API
        T1 a2; a2.p = A.floats((size_t)B * Tc); a2.B = B; a2.C = 1; a2.T = Tc; a2.ld = Tc; a2.halo = 0; a2.bs = Tc;
        T1 a1 = pl.audio;
        pl.ops.push_back([=](hipStream_t s) { HIPCHK(hipMemcpy2DAsync(a2.p, (size_t)Tc * 4, a1.p, (size_t)a1.bs * 4, (size_t)Tc * 4, B, hipMemcpyDeviceToDevice, s)); });
        pl.audio = a2;
    }
    add_stamp(pl, "sy.audio");
}

}  // namespace rvc
