// model_cv.hip -- ContentVec / HuBERT-base feature extractor as a plan (reference: rvc/src/rvc.rs:81-97, ort::Session::run at rvc.rs:92)
#include "engine_int.h"
#include "contentvec.hip.h"

namespace rvc {

// ------------------------------- the model as loaded (struct ModelCV: engine_int.h) ------------------------------------------
ConvW ModelCV::fold_ln(const float *w, const float *bias, int M, int K, const float *g, const float *beta, float **wsum_dev)
{
    std::vector<float> wf((size_t)M * K), bf(M), ws(M);
    for (int m = 0; m < M; m++) {
        double sb = bias ? bias[m] : 0.0, sw = 0.0;
        for (int k = 0; k < K; k++) {
            const float v = w[(size_t)m * K + k] * g[k];
            wf[(size_t)m * K + k] = v;
            sb += (double)w[(size_t)m * K + k] * beta[k];
            sw += v;
        }
        bf[m] = (float)sb; ws[m] = (float)sw;
    }
    *wsum_dev = upload_f(ws);
    return prep_conv(wf.data(), bf.data(), M, K, 1, 1);
}
ModelCV::ModelCV(const Blob &b)
{
    conv_dim = b.icfg("conv_dim"); embed = b.icfg("embed"); heads = b.icfg("heads"); ffn = b.icfg("ffn");
    run_layers = b.icfg("run_layers"); pos_k = b.icfg("pos_k"); pos_groups = b.icfg("pos_groups"); out_dim = b.icfg("out_dim");
    int cin = 1;
    for (int i = 0; i < 7; i++) {
        conv_k[i] = b.icfg(fmt("conv_k%d", i)); conv_s[i] = b.icfg(fmt("conv_s%d", i));
        conv[i] = prep_conv(b.w(fmt("cv.conv%d.w", i)), nullptr, conv_dim, cin, conv_k[i], 1);
        cin = conv_dim;
    }
    auto own = [&](const std::string &n) { float *p = dv(b, n); owned.push_back(p); return p; };
    conv0_raw = own("cv.conv0.w");
    gn_g = own("cv.gn.g"); gn_b = own("cv.gn.b"); ln0_g = own("cv.ln0.g"); ln0_b = own("cv.ln0.b");
    proj = prep_conv(b.w("cv.proj.w"), b.w("cv.proj.b"), embed, conv_dim, 1, 1);
    pos = prep_conv(b.w("cv.pos.w"), b.w("cv.pos.b"), embed, embed, pos_k, pos_groups);
    encln_g = own("cv.enc_ln.g"); encln_b = own("cv.enc_ln.b");
    const int E = embed;
    for (int l = 0; l < run_layers; l++) {
        Layer L;
        std::vector<float> w((size_t)3 * E * E), bb((size_t)3 * E);
        const char *nm[3] = {"q", "k", "v"};
        for (int j = 0; j < 3; j++) {
            memcpy(&w[(size_t)j * E * E], b.w(fmt("cv.l%d.", l) + nm[j] + ".w"), (size_t)E * E * 4);
            memcpy(&bb[(size_t)j * E], b.w(fmt("cv.l%d.", l) + nm[j] + ".b"), (size_t)E * 4);
        }
        L.qkv = prep_conv(w.data(), bb.data(), 3 * E, E, 1, 1);
        L.o = prep_conv(b.w(fmt("cv.l%d.o.w", l)), b.w(fmt("cv.l%d.o.b", l)), E, E, 1, 1);
        L.ff1 = prep_conv(b.w(fmt("cv.l%d.ff1.w", l)), b.w(fmt("cv.l%d.ff1.b", l)), ffn, E, 1, 1);
        L.ff2 = prep_conv(b.w(fmt("cv.l%d.ff2.w", l)), b.w(fmt("cv.l%d.ff2.b", l)), E, ffn, 1, 1);
        L.ln1_g = own(fmt("cv.l%d.ln1.g", l)); L.ln1_b = own(fmt("cv.l%d.ln1.b", l));
        L.ln2_g = own(fmt("cv.l%d.ln2.g", l)); L.ln2_b = own(fmt("cv.l%d.ln2.b", l));
        if (E >= 256 && E % 64 == 0 && ffn % 64 == 0 && !test_opt("RVC_NO_LN_FUSE")) {
            has_folded = true;
            L.ff1_f = fold_ln(b.w(fmt("cv.l%d.ff1.w", l)), b.w(fmt("cv.l%d.ff1.b", l)), ffn, E, b.w(fmt("cv.l%d.ln1.g", l)), b.w(fmt("cv.l%d.ln1.b", l)), &L.ff1_wsum);
            if (l > 0) L.qkv_f = fold_ln(w.data(), bb.data(), 3 * E, E, b.w(fmt("cv.l%d.ln2.g", l - 1)), b.w(fmt("cv.l%d.ln2.b", l - 1)), &L.qkv_wsum);
            else L.qkv_f = fold_ln(w.data(), bb.data(), 3 * E, E, b.w("cv.enc_ln.g"), b.w("cv.enc_ln.b"), &L.qkv_wsum);      // layer 0: the encoder's input LayerNorm
        }
        layers.push_back(L);
    }
    if (out_dim != E) final_proj = prep_conv(b.w("cv.final_proj.w"), b.w("cv.final_proj.b"), out_dim, E, 1, 1);
    if (has_folded && conv_dim % 64 == 0) proj_f = fold_ln(b.w("cv.proj.w"), b.w("cv.proj.b"), embed, conv_dim, b.w("cv.ln0.g"), b.w("cv.ln0.b"), &proj_wsum);
    weight_bytes = b.bytes();
}
ModelCV::~ModelCV()
{
    for (auto &c : conv) free_conv(c);
    free_conv(proj); free_conv(pos); free_conv(final_proj); free_conv(proj_f);
    if (proj_wsum) wfree(proj_wsum);
    for (auto &L : layers) {
        free_conv(L.qkv); free_conv(L.o); free_conv(L.ff1); free_conv(L.ff2); free_conv(L.qkv_f); free_conv(L.ff1_f);
        if (L.qkv_wsum) wfree(L.qkv_wsum);
        if (L.ff1_wsum) wfree(L.ff1_wsum);
    }
    for (float *p : owned) wfree(p);
}

// ------------------------------- ContentVec ------------------------------------------
// First layer: Conv1d(1 -> C, k taps, no bias) + GroupNorm (one group per channel: statistics over time) + GELU on the raw input x [B][1][L] into
// y [B][C][To].  Three paths: the fused multi-channel kernel (10 taps, To <= 8192, an even channel count), the fused one-channel kernel (<= 16 taps,
// To <= 8192) and the generic convolution followed by groupnorm_gelu_kernel.  The path taken is recorded (rvc_debug_last_kernel: "conv0_multi4|8",
// "conv0_one8|16|32", "conv0_generic"); the test hook RVC_CONV0_KERNEL = multi | one | generic replaces the rules' choice where that path is
// eligible, and is refused (ShapeError, nothing queued) elsewhere.
void add_conv0_front(Plan &pl, const ConvW &cw, const float *w_raw, const float *gn_g, const float *gn_b, int kt, int st, const T1 &x, const T1 &y)
{
    const int B = x.B, C = y.C, To = y.T;
    const bool fuse_ok = kt <= 16 && To <= 32 * 256 && w_raw != nullptr;
    // 16 channels per workgroup share one register copy of the input samples at many streams; one stream: 2 (256 workgroups of
    // 1024 threads, half the strided gathers: 42.8 -> ~15 us, 25-30 us off the ContentVec branch; 4 and 8 measured the same / worse)
    int cpw = B >= 16 ? 16 : (B >= 4 ? 4 : 2);
    if (const char *f = tune_env("RVC_CONV0_CPW")) cpw = std::max(1, atoi(f));      // tuning aid
    while (cpw > 1 && C % cpw) cpw >>= 1;
    const bool multi_ok = fuse_ok && kt == 10 && To <= 8 * 1024 && cpw > 1;
    const char *path = fuse_ok && !tune_env("RVC_NO_CONV0_FUSE") ? (multi_ok && !test_opt("RVC_NO_CONV0_MULTI") ? "multi" : "one") : "generic";
    if (const char *f = test_opt("RVC_CONV0_KERNEL")) {
        const bool known = !strcmp(f, "multi") || !strcmp(f, "one") || !strcmp(f, "generic");
        if (!known) throw ShapeError(std::string("RVC_CONV0_KERNEL: unknown variant '") + f + "'");
        if ((!strcmp(f, "multi") && !multi_ok) || (!strcmp(f, "one") && !fuse_ok)) throw ShapeError(std::string("RVC_CONV0_KERNEL: variant '") + f + "' is not eligible for this shape");
        path = !strcmp(f, "multi") ? "multi" : (!strcmp(f, "one") ? "one" : "generic");
    }
    if (path[0] != 'g') {
        // fused: conv (Cin = 1) + per-channel GroupNorm + GELU, outputs held in registers between the passes
        dim3 grid(C, B);
        const float *w0 = w_raw, *gg = gn_g, *bb = gn_b;
        const float *ain = x.p; const long long abs_ = x.bs;
        const int nt = (To + 255) / 256;
        Plan *plp = &pl;
        if (path[0] == 'm') {
            dim3 gridm(C / cpw, B);
            const int nt1k = (To + 1023) / 1024;
            snprintf(g_last_kernel, sizeof g_last_kernel, "conv0_multi%d", nt1k <= 4 ? 4 : 8);
            pl.ops.push_back([=](hipStream_t s) {
                const float *in_ = plp->cur_in ? plp->cur_in : ain;      // a device-resident caller's buffer is read in place
                if (nt1k <= 4) hipLaunchKernelGGL((conv0_gn_gelu_multi_kernel<4, 10>), gridm, dim3(1024), 0, s, in_, abs_, w0, st, gg, bb, y.p, To, y.ld, y.bs, cpw);
                else hipLaunchKernelGGL((conv0_gn_gelu_multi_kernel<8, 10>), gridm, dim3(1024), 0, s, in_, abs_, w0, st, gg, bb, y.p, To, y.ld, y.bs, cpw);
            });
        } else {
            snprintf(g_last_kernel, sizeof g_last_kernel, "conv0_one%d", nt <= 8 ? 8 : (nt <= 16 ? 16 : 32));
            pl.ops.push_back([=](hipStream_t s) {
                const float *in_ = plp->cur_in ? plp->cur_in : ain;
                if (nt <= 8) hipLaunchKernelGGL((conv0_gn_gelu_kernel<8>), grid, dim3(256), 0, s, in_, abs_, w0, kt, st, gg, bb, y.p, To, y.ld, y.bs);
                else if (nt <= 16) hipLaunchKernelGGL((conv0_gn_gelu_kernel<16>), grid, dim3(256), 0, s, in_, abs_, w0, kt, st, gg, bb, y.p, To, y.ld, y.bs);
                else hipLaunchKernelGGL((conv0_gn_gelu_kernel<32>), grid, dim3(256), 0, s, in_, abs_, w0, kt, st, gg, bb, y.p, To, y.ld, y.bs);
            });
        }
        add_tap(pl, "cv.conv0", y);
        return;
    }
    ConvOpts o; o.act = ACT_NONE;
    pl.in_direct_ok = false;      // (the generic convolution bakes its input pointer: this plan keeps the staging copy)
    add_conv1d(pl, cw, x, y, st, 0, 1, o);
    snprintf(g_last_kernel, sizeof g_last_kernel, "conv0_generic");
    dim3 grid(C, B);
    pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(groupnorm_gelu_kernel, grid, dim3(256), 0, s, y.p, gn_g, gn_b, y.T, y.ld, y.bs); });
    add_tap(pl, "cv.conv0", y);
}

T1 build_contentvec(rvc_engine *e, Plan &pl, int B, size_t L)
{
    ModelCV &m = *e->cv;
    Arena &A = pl.arena;
    T1 x; x.p = pl.d_in; x.B = B; x.C = 1; x.T = (int)L; x.ld = (int)L; x.halo = 0; x.bs = (long long)L;
    int T = (int)L;
    for (int i = 0; i < 7; i++) {
        int To = (T - m.conv_k[i]) / m.conv_s[i] + 1;
        T1 y = make_t1(A, B, m.conv_dim, To, 0);
        if (i == 0) {
            add_conv0_front(pl, m.conv[0], m.conv0_raw, m.gn_g, m.gn_b, m.conv_k[0], m.conv_s[0], x, y);
            x = y; T = To;
            continue;
        }
        ConvOpts o; o.act = ACT_GELU;
        add_conv1d(pl, m.conv[i], x, y, m.conv_s[i], 0, 1, o);
        x = y; T = To;
    }
    add_tap(pl, "cv.feat", x);
    const bool fuse_ln = B <= LN_FOLD_MAX_STREAMS && m.has_folded && !pl.key.plain_plan && !test_opt("RVC_NO_LN_FUSE");
    const int E = m.embed;
    T1 h = make_t1(A, B, E, T, m.pos_k / 2);
    if (fuse_ln && m.proj_wsum) { ConvOpts o; o.ln_wsum = m.proj_wsum; o.ln_rows = m.conv_dim; add_conv1d(pl, m.proj_f, x, h, 1, 0, 1, o); }
    else {
    add_layernorm(pl, x, m.ln0_g, m.ln0_b);
    add_conv1d(pl, m.proj, x, h, 1, 0, 1);
    }
    add_tap(pl, "cv.proj", h);
    T1 h2 = make_t1(A, B, E, T, 0);
    { ConvOpts o; o.act = ACT_GELU; o.res = h.p; o.res_cs = h.ld; o.res_bs = h.bs; add_conv1d(pl, m.pos, h, h2, 1, m.pos_k / 2, 1, o); }
    if (!fuse_ln) add_layernorm(pl, h2, m.encln_g, m.encln_b);      // (folded: layer 0 consumes the not yet normalised sum, see below)
    add_tap(pl, fuse_ln ? "cv.pos.raw" : "cv.pos", h2);
    T1 qkv = make_t1(A, B, 3 * E, T, 0), att = make_t1(A, B, E, T, 0), ff = make_t1(A, B, m.ffn, T, 0);
    // One stream: the 2 LayerNorm launches of a layer are folded into the GEMMs around them (h2 then holds the NOT yet normalised sum;
    // `raw` says so, with the pending LayerNorm's scale / shift and the buffer its column statistics are published in)
    bool raw = fuse_ln; const float *raw_g = m.encln_g, *raw_b = m.encln_b; float *raw_st = nullptr;
    for (int l = 0; l < m.run_layers; l++) {
        ModelCV::Layer &Ly = m.layers[l];
        if (fuse_ln) {
            float *st_a = A.floats((size_t)2 * T + 16);
            if (raw) { ConvOpts o; o.ln_wsum = Ly.qkv_wsum; o.ln_stats_out = st_a; o.ln_rows = E; add_conv1d(pl, Ly.qkv_f, h2, qkv, 1, 0, 1, o); raw_st = st_a; }
            else add_conv1d(pl, Ly.qkv, h2, qkv, 1, 0, 1);
        } else
        { ConvOpts o; o.bf3 = pl.key.bf3; add_conv1d(pl, Ly.qkv, h2, qkv, 1, 0, 1, o); }
        add_attention(pl, qkv, att, m.heads);
        if (fuse_ln) {
            float *st_1 = A.floats((size_t)2 * T + 16);
            {   // attention output projection + residual; the residual is LayerNorm2 of the previous layer when that one is still pending
                ConvOpts o; o.res = h2.p; o.res_cs = h2.ld; o.res_bs = h2.bs;
                if (raw) { o.ln_stats_in = raw_st; o.ln_g = raw_g; o.ln_b = raw_b; }
                add_conv1d(pl, Ly.o, att, h2, 1, 0, 1, o);
            }
            { ConvOpts o; o.act = ACT_GELU; o.ln_wsum = Ly.ff1_wsum; o.ln_stats_out = st_1; o.ln_rows = E; add_conv1d(pl, Ly.ff1_f, h2, ff, 1, 0, 1, o); }     // LayerNorm1 folded
            { ConvOpts o; o.res = h2.p; o.res_cs = h2.ld; o.res_bs = h2.bs; o.ln_stats_in = st_1; o.ln_g = Ly.ln1_g; o.ln_b = Ly.ln1_b; add_conv1d(pl, Ly.ff2, ff, h2, 1, 0, 1, o); }
            if (l + 1 < m.run_layers) { raw = true; raw_g = Ly.ln2_g; raw_b = Ly.ln2_b; }
            else { add_layernorm(pl, h2, Ly.ln2_g, Ly.ln2_b); raw = false; }
        } else {
        { ConvOpts o; o.bf3 = pl.key.bf3; o.res = h2.p; o.res_cs = h2.ld; o.res_bs = h2.bs; add_conv1d(pl, Ly.o, att, h2, 1, 0, 1, o); }
        add_layernorm(pl, h2, Ly.ln1_g, Ly.ln1_b);
        { ConvOpts o; o.bf3 = pl.key.bf3; o.act = ACT_GELU; add_conv1d(pl, Ly.ff1, h2, ff, 1, 0, 1, o); }
        { ConvOpts o; o.bf3 = pl.key.bf3; o.res = h2.p; o.res_cs = h2.ld; o.res_bs = h2.bs; add_conv1d(pl, Ly.ff2, ff, h2, 1, 0, 1, o); }
        add_layernorm(pl, h2, Ly.ln2_g, Ly.ln2_b);
        }
        if (pl.key.with_taps) { char nm[32]; snprintf(nm, sizeof nm, raw ? "cv.l%d.raw" : "cv.l%d", l); add_tap(pl, nm, h2); } else if (l % 4 == 3) add_stamp(pl, "cv.l4");
    }
    T1 out = h2;
    if (m.out_dim != E) { out = make_t1(A, B, m.out_dim, T, 0); add_conv1d(pl, m.final_proj, h2, out, 1, 0, 1); }
    add_tap(pl, "cv.out", out);
    pl.T = T; pl.C = m.out_dim;
    return out;
}

}  // namespace rvc
