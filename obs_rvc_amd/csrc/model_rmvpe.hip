// model_rmvpe.hip -- RMVPE f0 estimator (mel front end, U-Net, BiGRU, salience) and the decode / pitch-cache step as a plan (reference: rvc/src/f0/rmvpe.rs:118-133, 225-248; rvc/src/rvc.rs:111-131, 167-180)
#include "engine_int.h"
#include "rmvpe.hip.h"
#include "rmblock.hip.h"
#include "f0_hybrid.hip.h"

namespace rvc {

// ------------------------------- the model as loaded (struct ModelRM, ResBlockW: engine_int.h) ------------------------------------------
// -> fragment-order panel of a [co][ci * taps] convolution weight for rm_block_kernel
static std::vector<float> rm_block_panel(const float *w, int co, int ci, int taps)
{
    const int c16 = (ci + 15) / 16 * 16, steps = c16 / 4, MT = co / 16;
    std::vector<float> pk((size_t)taps * steps * MT * 64, 0.f);
    for (int t = 0; t < taps; t++)
        for (int c4 = 0; c4 < steps; c4++)
            for (int mt = 0; mt < MT; mt++)
                for (int l = 0; l < 64; l++) {
                    const int m = mt * 16 + (l & 15), c = c4 * 4 + (l >> 4);
                    if (c < ci) pk[(((size_t)t * steps + c4) * MT + mt) * 64 + l] = w[(size_t)m * ci * taps + (size_t)c * taps + t];
                }
    return pk;
}
ResBlockW make_res_block(const float *w1, const float *b1, const float *w2, const float *b2, const float *wsc, const float *bsc, int ci, int co)
{
    ResBlockW r; r.ci = ci; r.co = co;
    r.c1 = prep_conv(w1, b1, co, ci, 9, 1);
    r.c2 = prep_conv(w2, b2, co, co, 9, 1);
    if (wsc) {
        r.has_sc = true; r.sc = prep_conv(wsc, bsc, co, ci, 1, 1);
        std::vector<float> pb(b1, b1 + co);
        pb.insert(pb.end(), bsc, bsc + co);
        r.pair_bias = upload_f(pb);
    }
    if ((co == 16 || co == 32) && ci <= 64) {
        std::vector<float> all = rm_block_panel(w1, co, ci, 9);
        const size_t o2 = all.size();
        { std::vector<float> t = rm_block_panel(w2, co, co, 9); all.insert(all.end(), t.begin(), t.end()); }
        const size_t o3 = all.size();
        if (r.has_sc) { std::vector<float> t = rm_block_panel(wsc, co, ci, 1); all.insert(all.end(), t.begin(), t.end()); }
        all.resize((all.size() + 31) / 32 * 32, 0.f);
        r.f_w1 = upload_f(all); r.f_w2 = r.f_w1 + o2; r.f_sc = r.has_sc ? r.f_w1 + o3 : nullptr; r.f_lines = (int)(all.size() / 32);
    }
    return r;
}
void free_res_block(ResBlockW &r)
{
    free_conv(r.c1); free_conv(r.c2); free_conv(r.sc);
    if (r.pair_bias) wfree(r.pair_bias);
    if (r.f_w1) wfree(r.f_w1);
    r.pair_bias = nullptr; r.f_w1 = r.f_w2 = r.f_sc = nullptr; r.f_lines = 0;
}
void gru_prep_whh(const float *const whh_dir[2], int H, std::vector<float> &whhT, std::vector<float> &whh)
{
    whhT.resize((size_t)2 * H * 3 * H); whh.resize((size_t)2 * 3 * H * H);
    for (int d = 0; d < 2; d++) {
        const float *w = whh_dir[d];
        for (int r = 0; r < 3 * H; r++) for (int j = 0; j < H; j++) whhT[((size_t)d * H + j) * 3 * H + r] = w[(size_t)r * H + j];
        memcpy(&whh[(size_t)d * 3 * H * H], w, (size_t)3 * H * H * sizeof(float));
    }
}
ResBlockW ModelRM::block(const Blob &b, const std::string &pre, int ci, int co)
{
    const bool sc = ci != co;
    return make_res_block(b.w(pre + "c1.w"), b.w(pre + "c1.b"), b.w(pre + "c2.w"), b.w(pre + "c2.b"), sc ? b.w(pre + "sc.w") : nullptr, sc ? b.w(pre + "sc.b") : nullptr, ci, co);
}
ModelRM::ModelRM(const Blob &b)
{
    en_out = b.icfg("en_out"); levels = b.icfg("levels"); n_blocks = b.icfg("n_blocks"); inter_layers = b.icfg("inter_layers");
    n_mels = b.icfg("n_mels"); gru_hidden = b.icfg("gru_hidden"); n_out = b.icfg("n_out");
    bn_scale = b.w("rm.bn0")[0]; bn_shift = b.w("rm.bn0")[1];
    int ci = 1, co = en_out;
    for (int lv = 0; lv < levels; lv++) {
        std::vector<ResBlockW> v;
        for (int j = 0; j < n_blocks; j++) v.push_back(block(b, fmt("rm.enc%d.b%d.", lv, j), j == 0 ? ci : co, co));
        enc.push_back(v);
        ci = co; co *= 2;
    }
    for (int lv = 0; lv < inter_layers; lv++) {
        std::vector<ResBlockW> v;
        for (int j = 0; j < n_blocks; j++) v.push_back(block(b, fmt("rm.int%d.b%d.", lv, j), j == 0 ? (lv == 0 ? ci : co) : co, co));
        inter.push_back(v);
    }
    ci = co;
    for (int lv = 0; lv < levels; lv++) {
        co = ci / 2;
        up.push_back(prep_convT2d(b.w(fmt("rm.dec%d.up.w", lv)), b.w(fmt("rm.dec%d.up.b", lv)), ci, co));
        std::vector<ResBlockW> v;
        for (int j = 0; j < n_blocks; j++) v.push_back(block(b, fmt("rm.dec%d.b%d.", lv, j), j == 0 ? 2 * co : co, co));
        dec.push_back(v);
        ci = co;
    }
    cnn = prep_conv(b.w("rm.cnn.w"), b.w("rm.cnn.b"), 3, en_out, 9, 1);
    const int H = gru_hidden, I = 3 * n_mels;
    std::vector<float> wih((size_t)6 * H * I), bih((size_t)6 * H), bh((size_t)6 * H);
    const char *sfx[2] = {"f", "b"};
    const float *whh_dir[2];
    for (int d = 0; d < 2; d++) {
        memcpy(&wih[(size_t)d * 3 * H * I], b.w(std::string("rm.gru.w_ih_") + sfx[d]), (size_t)3 * H * I * 4);
        memcpy(&bih[(size_t)d * 3 * H], b.w(std::string("rm.gru.b_ih_") + sfx[d]), (size_t)3 * H * 4);
        memcpy(&bh[(size_t)d * 3 * H], b.w(std::string("rm.gru.b_hh_") + sfx[d]), (size_t)3 * H * 4);
        whh_dir[d] = b.w(std::string("rm.gru.w_hh_") + sfx[d]);
    }
    gru_ih = prep_conv(wih.data(), bih.data(), 6 * H, I, 1, 1);
    {
        std::vector<float> wt, wr;
        gru_prep_whh(whh_dir, H, wt, wr);
        whhT = upload_f(wt); bhh = upload_f(bh); whh = upload_f(wr);
    }
    fc = prep_conv(b.w("rm.fc.w"), b.w("rm.fc.b"), n_out, 2 * H, 1, 1);
    weight_bytes = b.bytes();
}
ModelRM::~ModelRM()
{
    auto fb = [](std::vector<std::vector<ResBlockW>> &vv) { for (auto &v : vv) for (auto &r : v) free_res_block(r); };
    fb(enc); fb(inter); fb(dec);
    for (auto &u : up) free_conv(u);
    free_conv(cnn); free_conv(gru_ih); free_conv(fc);
    if (whhT) wfree(whhT);
    if (bhh) wfree(bhh);
    if (whh) wfree(whh);
}

// One launch per ConvBlockRes on the shallow levels (rm_block_kernel, rmblock.hip.h): few streams only -- there the f0 branch is a chain of dependent
// 5-8 us launches on its own CU partition and the block's halo recomputation costs nothing that matters; with many streams folded into a launch the two
// convolutions fill the chip by themselves and keep the implicit-GEMM kernels.  Test hook RVC_RM_FUSE = 0: never, 2: at any stream count, 3: by the rule, but
// build_rmvpe folds no pooling into a block (neither the AvgPool2d in front of a level's first block nor the pooled second output of its last).  false = not taken.
// pool_src != nullptr: the block's input is AvgPool2d(2, 2) of that tensor, averaged while the tile is staged (the pooling launch in front of the block disappears);
// dry: eligibility only, nothing queued.  A queued block is recorded (rvc_debug_last_kernel: "rmb_<MT>_<NT1>_<NT2>", "+pool_in" / "+pool_out" for the folded poolings)
bool add_rm_block_fused(Plan &pl, const ResBlockW &w, const T2 &x, const T2 &out, const ResBlockW *next, const T2 *pool_src, bool dry, const T2 *pool_dst)
{
    const int mode = test_opt_int("RVC_RM_FUSE", 1);
    if (!w.f_w1 || mode == 0 || (!pl.rm_fuse && mode != 2)) return false;
    if (x.C != w.ci || out.C != w.co || out.H != x.H || out.W != x.W || (!w.has_sc && w.ci != w.co)) return false;
    const int MT = w.co / 16;
    RmBlockP q{};
    q.x = x.p; q.y = out.p; q.Cin = w.ci; q.Cin4 = (w.ci + 15) / 16 * 4; q.Cout = w.co;
    q.H = x.H; q.W = x.W;
    // output tile per workgroup: 128 / 32 / 8 pixels for 16 / 32 / 64 channels (32 workgroups per stream at the 32 x 128 mel image: one per CU of the
    // f0 partition); the y1 tile must fit the waves' n-tiles: ceil((TH + 2)(TW + 2) / 16) <= 4 * (4 / MT)
    q.TH = MT == 1 ? 8 : (MT == 2 ? 4 : 2); q.TW = MT == 1 ? 16 : (MT == 2 ? 8 : 4);
    q.TH = std::min(q.TH, x.H); q.TW = std::min(q.TW, x.W);
    // n-tiles per wave of the two convolutions (template parameters of the kernel): 3 / 2 for 16 channels (12 and 8 tiles over four waves), 2 / 1 for 32 and 64
    const int NT1 = MT == 1 ? 3 : 2, NT2 = MT == 1 ? 2 : 1, NWN = 4 / MT;
    if (MT > 2) return false;          // (64 channels: every workgroup would stream 2 x 147 KB of weights for 8 output pixels -- measured 19 us against 11.6 for the two launches)
    if (((q.TH + 2) * (q.TW + 2) + 15) / 16 > NT1 * NWN || (q.TH * q.TW + 15) / 16 > NT2 * NWN || (q.TH + 4) * (q.TW + 4) > 256) return false;      // (the staging gives every tile position a thread)
    q.tiles_x = (x.W + q.TW - 1) / q.TW;
    const int tiles = q.tiles_x * ((x.H + q.TH - 1) / q.TH);
    q.x_ld = x.ld; q.x_cs = x.cs; q.x_bs = x.bs; q.y_ld = out.ld; q.y_cs = out.cs; q.y_bs = out.bs;
    if (pool_src) { q.x = pool_src->p; q.x_ld = pool_src->ld; q.x_cs = pool_src->cs; q.x_bs = pool_src->bs; q.pool = 1; }
    q.w1 = w.f_w1; q.w2 = w.f_w2; q.wsc = w.has_sc ? w.f_sc : nullptr;
    q.b1 = w.c1.bias; q.b2 = w.c2.bias; q.bsc = w.has_sc ? w.sc.bias : nullptr;
    q.wlines = w.f_lines; q.wnext = next ? next->f_w1 : nullptr; q.wnext_lines = next ? next->f_lines : 0;
    if (q.wlines > 1536 || q.wnext_lines > 1536) return false;
    auto stride = [](int n) { int v = n / 32 * 32 + 16; return v < n ? v + 32 : v; };      // >= n and 16 mod 32: the k-slots of a read alternate between the two bank halves
    q.XS = stride((q.TH + 4) * (q.TW + 4)); q.YS = stride((q.TH + 2) * (q.TW + 2));
    const size_t lds = ((size_t)q.Cin4 * 4 * q.XS + (size_t)q.Cout * q.YS) * sizeof(float);
    if (lds > 64 * 1024) return false;
    if (pool_dst) {          // second output: the pooled tensor (tiles of eight columns; even image and tile sizes)
        if (q.TW != 8 || (q.TH & 1) || (x.H & 1) || (x.W & 1) || pool_dst->H * 2 != x.H || pool_dst->W * 2 != x.W || pool_dst->C != w.co) return false;
        q.ypool = pool_dst->p; q.p_ld = pool_dst->ld; q.p_cs = pool_dst->cs; q.p_bs = pool_dst->bs;
    }
    if (dry) return true;
    q.tiles = tiles;
    const dim3 grid((unsigned)(tiles + (q.wnext ? 1 : 0)), (unsigned)x.B);
    const double flops = 2.0 * w.co * (double)x.H * x.W * (9.0 * w.ci + 9.0 * w.co + (w.has_sc ? w.ci : 0)) * x.B;
    pl.igemm_flops += flops; pl.n_igemm++;
    Plan *plp = &pl;
    { char d[176]; snprintf(d, sizeof d, "rmb M=%d N=%d K=%d B=%d nph=1 tile=%dx%d grid=%ux%u lds=%zu sc=%d", w.co, x.H * x.W, 9 * w.ci + 9 * w.co + (w.has_sc ? w.ci : 0), x.B, q.TH, q.TW, grid.x, grid.y, lds, (int)w.has_sc); pl.descs.push_back(d); }
    const int desc_id = (int)pl.descs.size() - 1;
    snprintf(g_last_kernel, sizeof g_last_kernel, "rmb_%d_%d_%d%s%s", MT, NT1, NT2, q.pool ? "+pool_in" : "", q.ypool ? "+pool_out" : "");
    pl.ops.push_back([=](hipStream_t s) {
        const ProfEvent *pe = plp->prof_slot(flops, 0, desc_id);
        hipEvent_t ea = pe ? pe->a : nullptr, eb = pe ? pe->b : nullptr;
#define RVC_RMB_LAUNCH(MT_, N1_, N2_)                                                                                         \
        { if (ea) hipExtLaunchKernelGGL((rm_block_kernel<MT_, N1_, N2_>), grid, dim3(256), (uint32_t)lds, s, ea, eb, 0, q);  \
          else hipLaunchKernelGGL((rm_block_kernel<MT_, N1_, N2_>), grid, dim3(256), lds, s, q); }
        if (MT == 1) RVC_RMB_LAUNCH(1, 3, 2) else if (MT == 2) RVC_RMB_LAUNCH(2, 2, 1) else RVC_RMB_LAUNCH(4, 2, 1)
#undef RVC_RMB_LAUNCH
    });
    return true;
}

static void add_conv2d_with_shortcut(Plan &pl, const ResBlockW &w, const T2 &x, const T2 &y1, const T2 &out)
{
    if (x.H != y1.H || x.W != y1.W || out.H != x.H || out.W != x.W || y1.cs != out.cs || y1.ld != out.ld || (x.B > 1 && y1.bs != out.bs)) throw ShapeError("conv2d + shortcut: layouts differ");
    const ConvW &c1 = w.c1, &sc = w.sc;
    IgemmP p{};
    p.x = x.p; p.y = y1.p;
    p.M = c1.M; p.N = x.H * x.W;
    p.NW = x.W; p.x_hs = x.ld; p.x_ws = 1; p.y_hm = 1; p.y_ws = 1; p.OW = y1.W;
    p.x_bs = x.bs; p.y_bs = y1.bs; p.y_cs = y1.cs; p.y_rs = y1.ld;
    ConvOpts o; o.act = ACT_RELU;
    fill_epilogue(p, c1, o);
    p.bias = w.pair_bias;
    std::vector<int> koff;
    std::vector<PhaseD> ph(2);
    ph[0] = PhaseD{}; ph[1] = PhaseD{};
    // phase 0: the 3x3 convolution (one-row images: only the middle tap row can hit data, see add_conv2d)
    if (x.H == 1 && !c1.host_w.empty() && !tune_env("RVC_NO_TAP_PRUNE")) {
        const int K3 = c1.Cin * 3, Kp3 = round16(K3);
        std::vector<float> panel((size_t)c1.M * Kp3, 0.f);
        for (int mo = 0; mo < c1.M; mo++)
            for (int ci = 0; ci < c1.Cin; ci++)
                for (int kw = 0; kw < 3; kw++) panel[(size_t)mo * Kp3 + ci * 3 + kw] = c1.host_w[(size_t)mo * c1.K + ci * 9 + 3 + kw];
        float *dw = upload_fragments(panel, 1, c1.M, Kp3, 1);      // plan-lifetime copy
        pl.owned_dev.push_back(dw);
        p.w = dw; ph[0].nchunks = Kp3 / 16;
        koff.assign(Kp3, 0);
        for (int ci = 0; ci < c1.Cin; ci++) for (int kw = 0; kw < 3; kw++) koff[ci * 3 + kw] = ci * x.cs + (kw - 1);
    } else {
        p.w = c1.w; ph[0].nchunks = c1.Kp / 16;
        koff.assign(c1.Kp, 0);
        for (int ci = 0; ci < c1.Cin; ci++) for (int k = 0; k < 9; k++) koff[ci * 9 + k] = ci * x.cs + (k / 3 - 1) * x.ld + (k % 3 - 1);
    }
    // phase 1: the shortcut: its own weights (offset from phase 0's: both are device pointers of one flat address space), K, bias
    // slice, output tensor and (no) activation
    ph[1].w_off = sc.w - p.w;
    ph[1].nchunks = sc.Kp / 16;
    ph[1].koff_off = (int)koff.size();
    ph[1].bias_off = c1.M;
    ph[1].act_p1 = ACT_NONE + 1;
    ph[1].y_off = out.p - y1.p;
    const size_t base = koff.size();
    koff.resize(base + sc.Kp, 0);
    for (int ci = 0; ci < sc.Cin; ci++) koff[base + ci] = ci * x.cs;
    p.K = std::max(ph[0].nchunks, ph[1].nchunks) * 16;
    queue_igemm(pl, p, x.B, koff, ph);
}

// the unfused forms are recorded as "pair" / "plain" (rvc_debug_last_kernel)
T2 add_res_block(Plan &pl, const ResBlockW &w, const T2 &x, const T2 &out, const ResBlockW *next, const T2 *pool_src, const T2 *pool_dst)
{
    Arena &A = pl.arena;
    if (add_rm_block_fused(pl, w, x, out, (next && next->f_w1) ? next : nullptr, pool_src, false, pool_dst)) return out;
    if (pool_src || pool_dst) throw std::runtime_error("RMVPE: pooled input without the fused block");
    T2 y1 = make_t2(A, x.B, w.co, x.H, x.W);
    // few streams: the 3x3 convolution and the 1x1 shortcut read the same input -- one launch with two phases (own K, own output tensor,
    // own activation) instead of two dependent launches (11 blocks of RMVPE have a shortcut: 11 launches off the f0 branch)
    if (w.has_sc && w.pair_bias && x.B <= 4 && (x.B == 1 || y1.bs == out.bs) && !tune_env("RVC_NO_SC_MERGE")) {      // (one stream stride for both outputs)
        add_conv2d_with_shortcut(pl, w, x, y1, out);
        ConvOpts o; o.act = ACT_RELU; o.accumulate = true; add_conv2d(pl, w.c2, y1, out, o);
        snprintf(g_last_kernel, sizeof g_last_kernel, "pair");
        return out;
    }
    { ConvOpts o; o.act = ACT_RELU; add_conv2d(pl, w.c1, x, y1, o); }
    if (w.has_sc) {
        add_conv2d(pl, w.sc, x, out);
        ConvOpts o; o.act = ACT_RELU; o.accumulate = true; add_conv2d(pl, w.c2, y1, out, o);
    } else {
        ConvOpts o; o.act = ACT_RELU; o.res = x.p; o.res_cs = x.cs; o.res_bs = x.bs; o.res_rs = x.ld; add_conv2d(pl, w.c2, y1, out, o);
    }
    snprintf(g_last_kernel, sizeof g_last_kernel, "plain");
    return out;
}

// AvgPool2d(2, 2) of x [B][C][H][W] into p [B][C][H / 2][W / 2] as a launch of its own
void add_avgpool2(Plan &pl, const T2 &x, const T2 &p)
{
    const int co = p.C;
    dim3 grid((co * p.H * p.W + 255) / 256, x.B);
    pl.ops.push_back([=](hipStream_t s) {
        hipLaunchKernelGGL(avgpool2_kernel, grid, dim3(256), 0, s, x.p, x.ld, x.cs, x.bs, p.p, p.ld, p.cs, p.bs, co, p.H, p.W);
    });
}

// RMVPE's front end on the last `frame` of the n samples of each stream (audio [B][audio_bs]): the raw log-mel into mel [B][128][Tm] and, with the network's
// input affine, into the image img [B][1][Tm][128].  The engine's tables (window, twiddles, mel basis and bands) are used; an eager launch reads the
// caller's device buffer (Plan::cur_in) in place of `audio` when there is one.
void add_mel_frontend(rvc_engine *e, Plan &pl, int B, const float *audio, long long audio_bs, int n, int frame, int Tm, float *mel, const T2 &img, float bn_scale, float bn_shift)
{
    add_mel_frontend_tables(e, pl, B, audio, audio_bs, n, frame, Tm, mel, img, bn_scale, bn_shift, e->d_basis, e->d_band);
}
// ... the same launch on another filterbank: basis [128][513] and band [128][2] (first / one-past-last non-zero bin) on the device (FCPE's Slaney bank, model_fcpe.hip)
void add_mel_frontend_tables(rvc_engine *e, Plan &pl, int B, const float *audio, long long audio_bs, int n, int frame, int Tm, float *mel, const T2 &img, float bn_scale,
                             float bn_shift, const float *basis, const int *band)
{
    if (frame < 513 || frame > n || Tm < 1 || (long long)(Tm - 1) * 160 > (long long)frame) throw ShapeError("mel front end: frame out of range");   // (one reflection per side)
    MelP mp{};
    mp.audio = audio; mp.audio_bs = audio_bs; mp.n = n; mp.frame = frame; mp.Tm = Tm;
    mp.window = e->d_window; mp.twiddle = e->d_twiddle; mp.basis = basis; mp.band = band;
    mp.mel = mel; mp.img = img.p; mp.img_bs = img.bs; mp.img_ld = img.ld; mp.bn_scale = bn_scale; mp.bn_shift = bn_shift;
    dim3 grid(Tm, B);
    Plan *plp = &pl;
    pl.ops.push_back([=](hipStream_t s) { MelP m2 = mp; if (plp->cur_in) m2.audio = plp->cur_in; hipLaunchKernelGGL(mel_frontend_kernel, grid, dim3(256), 0, s, m2); });
}

T1 build_rmvpe(rvc_engine *e, Plan &pl, int B, size_t L, size_t frame16k, bool update_cache)
{
    ModelRM &m = *e->rm;
    Arena &A = pl.arena;
    // fused shallow blocks (rm_block_kernel): where the f0 branch runs on its own single-XCD partition -- up to four streams, and not the v1 engines of up to
    // three streams, whose branch has two XCDs (the kernel's 32 workgroups per stream and its L2 warming are sized for one: v1 at one stream measured 1.92 ->
    // 1.94 ms with it, v2 1.99 -> 1.965)
    pl.rm_fuse = e->partitioned && (g_ncu - e->cv_cus) * 8 == g_ncu && B <= 4;
    const size_t fr = 5120 * ((frame16k + 800 - 1) / 5120 + 1) - 160;     // rmvpe.rs:256
    if (fr > L) throw PanicError("input shorter than f0_extractor_frame");
    const int Tm = (int)(1 + fr / 160);
    if (Tm % 32 != 0) throw PanicError("mel frame count is not a multiple of 32 (rmvpe.rs:229-233 branch)");
    if (Tm > 1024) throw ShapeError("f0 window too long");
    pl.Tm = Tm;
    const int H0 = Tm, W0 = m.n_mels;
    if ((H0 >> m.levels) < 1 || (W0 >> m.levels) < 1) throw ShapeError("RMVPE: input too small for the U-Net depth");
    T2 img = make_t2(A, B, 1, H0, W0);
    float *d_mel = A.floats((size_t)B * 128 * Tm);
    add_mel_frontend(e, pl, B, pl.d_in, (long long)L, (int)L, (int)fr, Tm, d_mel, img, m.bn_scale, m.bn_shift);
    add_stamp(pl, "rm.mel0");
    if (pl.key.with_taps) { T1 t; t.p = d_mel; t.B = B; t.C = 128; t.T = Tm; t.ld = Tm; t.halo = 0; t.bs = 128LL * Tm; add_tap(pl, "rm.mel", t); }
    // encoder; every level's pre-pool output is written straight into the second half of the decoder's concat buffer
    std::vector<T2> cat(m.levels);
    {
        int H = H0, W = W0, co = m.en_out;
        for (int lv = 0; lv < m.levels; lv++) { cat[lv] = make_t2(A, B, 2 * co, H, W); H /= 2; W /= 2; co *= 2; }
    }
    T2 x = img;
    int H = H0, W = W0;
    T2 pool_from; bool pooled_in_block = false;         // the previous level's output when its pooling is folded into this level's first (fused) block
    for (int lv = 0; lv < m.levels; lv++) {
        const int co = m.enc[lv][0].co;
        T2 p = make_t2(A, B, co, H / 2, W / 2);
        // ... and a level whose LAST block is a fused block with eight-column tiles writes the pooled tensor as a second output of that block
        const bool next_takes_pool = lv + 1 < m.levels && (H % 2) == 0 && (W % 2) == 0 && test_opt_int("RVC_RM_FUSE", 1) != 3 &&
                                     [&]() { T2 o = p; o.C = m.enc[lv + 1][0].co; return add_rm_block_fused(pl, m.enc[lv + 1][0], p, o, nullptr, &x, true); }();
        bool pooled_by_block = false;
        for (int j = 0; j < m.n_blocks; j++) {
            T2 out = (j == m.n_blocks - 1) ? cat[lv].chans(co, co) : make_t2(A, B, co, H, W);
            const bool last = j == m.n_blocks - 1;
            const T2 xin = x;
            pooled_by_block = last && !next_takes_pool && test_opt_int("RVC_RM_FUSE", 1) != 3 && add_rm_block_fused(pl, m.enc[lv][j], xin, out, nullptr, (j == 0 && pooled_in_block) ? &pool_from : nullptr, true, &p);
            x = add_res_block(pl, m.enc[lv][j], xin, out, j + 1 < m.n_blocks ? &m.enc[lv][j + 1] : (lv + 1 < m.levels ? &m.enc[lv + 1][0] : nullptr), (j == 0 && pooled_in_block) ? &pool_from : nullptr,
                          pooled_by_block ? &p : nullptr);
        }
        if (pl.key.with_taps) { char nm[32]; snprintf(nm, sizeof nm, "rm.enc%d", lv); add_tap2(pl, nm, x); }
        // the next level's first block stages AvgPool2d(2, 2) of this level's output itself when it is a fused block (one more launch off the f0 branch)
        pooled_in_block = next_takes_pool;
        if (pooled_in_block) pool_from = x;
        else if (!pooled_by_block) add_avgpool2(pl, x, p);
        x = p; H /= 2; W /= 2;
    }
    for (int lv = 0; lv < m.inter_layers; lv++)
        for (int j = 0; j < m.n_blocks; j++) { T2 out = make_t2(A, B, m.inter[lv][j].co, H, W); x = add_res_block(pl, m.inter[lv][j], x, out); }
    add_tap2(pl, "rm.int", x);
    for (int lv = 0; lv < m.levels; lv++) {
        const int sl = m.levels - 1 - lv, co = m.up[lv].Cout;
        H *= 2; W *= 2;
        { ConvOpts o; o.act = ACT_RELU; add_convT2d(pl, m.up[lv], x, cat[sl].chans(0, co), o); }
        x = cat[sl];
        for (int j = 0; j < m.n_blocks; j++) { T2 out = make_t2(A, B, co, H, W); x = add_res_block(pl, m.dec[lv][j], x, out, j + 1 < m.n_blocks ? &m.dec[lv][j + 1] : (lv + 1 < m.levels ? &m.dec[lv + 1][0] : nullptr)); }
        if (pl.key.with_taps) { char nm[32]; snprintf(nm, sizeof nm, "rm.dec%d", lv); add_tap2(pl, nm, x); }
    }
    const int Hg = m.gru_hidden, I = 3 * m.n_mels;
    T1 feat = make_t1(A, B, I, Tm, 0), gi = make_t1(A, B, 6 * Hg, Tm, 0), gout = make_t1(A, B, 2 * Hg, Tm, 0), sal = make_t1(A, B, m.n_out, Tm, 0);
    if (H == Tm && W == m.n_mels && test_opt_int("RVC_RM_FUSE", 1) != 0) {
        // (round 6) the head convolution writes the GRU's input layout itself -- feat[c * n_mels + mel][t] = conv[c][t][mel]: channel stride n_mels rows, image row
        // (time) stride 1, image column (mel) stride one row of `feat` -- instead of an image and a transposing launch behind it
        T2 ft; ft.p = feat.p; ft.B = B; ft.C = 3; ft.H = H; ft.W = W; ft.cs = m.n_mels * feat.ld; ft.ld = 1; ft.bs = feat.bs;
        ConvOpts o; o.y_ws = feat.ld;
        add_conv2d(pl, m.cnn, x, ft, o);
    } else {
        T2 cn = make_t2(A, B, 3, H, W);
        add_conv2d(pl, m.cnn, x, cn);
        dim3 grid((3 * m.n_mels * Tm + 255) / 256, B); int nm = m.n_mels;
        pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(gru_input_kernel, grid, dim3(256), 0, s, cn.p, cn.ld, cn.cs, cn.bs, feat.p, feat.ld, feat.bs, Tm, nm); });
    }
    add_conv1d(pl, m.gru_ih, feat, gi, 1, 0, 1);
    add_gru(pl, gi, gout, Hg, m.whh, m.whhT, m.bhh, &e->d_state[0].status, (int)(sizeof(StreamState) / sizeof(int)));
    { ConvOpts o; o.act = ACT_SIGMOID; add_conv1d(pl, m.fc, gout, sal, 1, 0, 1, o); }
    if (pl.key.with_taps) { add_tap(pl, "rm.sal_ct", sal); add_tap(pl, "rm.gru_ct", gout); add_tap(pl, "rm.cnn_ct", feat); } else add_stamp(pl, "rm.sal");
    return sal;
}

// decode + pitch shift + pitch cache + get_f0_post (rmvpe.rs:118-133,243-248; rvc.rs:121,167-180; f0/mod.rs:7-12) of the salience sal [B][360][Tm] on the
// states st [B] (uppower, cache_pitchf, status): f0 [B][Tm]; update: the cache is shifted by `shift`, the new f0 inserted from cache_start on and
// R values from read_start sliced into pitchf / pitch [B][R].  f0_in [B][Tm] (another method's f0 in Hz, model_yin.hip): sal is not read, the decode is skipped
void add_pitch_post(Plan &pl, int B, const T1 &sal, int Tm, StreamState *st, const CallParams *cp, float *f0, bool update, long long shift, long long cache_start,
                    long long read_start, int R, float *pitchf, int *pitch, const float *f0_in)
{
    if ((!f0_in && (sal.C != 360 || sal.T != Tm)) || Tm < 1 || Tm > 1024) throw ShapeError("pitch decode: salience shape");
    PitchP pp{};
    pp.sal = sal.p; pp.sal_cs = sal.ld; pp.sal_bs = sal.bs; pp.Tm = Tm; pp.f0_in = f0_in;
    pp.st = st; pp.cp = cp; pp.f0 = f0; pp.threshold = 0.03f;   // rvc.rs:122
    if (update) {
        if (shift < 0 || shift > 1024 || Tm < 5) throw PanicError("pitch cache shift out of range");
        if (cache_start < 0 || read_start < 0 || read_start + R > 1024 || R < 0 || 3 + (1023 - cache_start) >= Tm) throw PanicError("pitch cache slice out of range");
        pp.pitchf = pitchf; pp.pitch = pitch;
        pp.shift = (int)shift; pp.cache_start = (int)cache_start; pp.read_start = (int)read_start; pp.R = R;
    } else {
        pp.R = 0; pp.shift = 0; pp.cache_start = 1 << 30; pp.read_start = 0; pp.pitchf = nullptr; pp.pitch = nullptr;
    }
    pp.update = update ? 1 : 0;
    pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(pitch_post_kernel, dim3(B), dim3(1024), 0, s, pp); });
}

void build_pitch_post(rvc_engine *e, Plan &pl, int B, const T1 &sal, bool update_cache, size_t frame16k, size_t hubert_length,
                             float **pitchf_out, int **pitch_out, const float *f0_in)
{
    Arena &A = pl.arena;
    const int Tm = pl.Tm;
    pl.d_f0 = A.floats((size_t)B * Tm);
    if (!update_cache) { add_pitch_post(pl, B, sal, Tm, e->d_state, e->d_cp, pl.d_f0, false, 0, 0, 0, 0, nullptr, nullptr, f0_in); return; }
    const int R = (int)pl.key.R;
    const size_t shift = frame16k / 160;                                   // rvc.rs:168
    if (shift > 1024 || Tm < 5) throw PanicError("pitch cache shift out of range");
    const long long cache_start = 1024 + 4 - Tm;                            // rvc.rs:172
    const long long read_start = 1024 - (long long)hubert_length + pl.key.skip_head;   // rvc.rs:176
    if (cache_start < 0 || read_start < 0 || read_start + R > 1024) throw PanicError("pitch cache slice out of range");
    float *pitchf = A.floats((size_t)B * R);
    int *pitch = (int *)A.alloc((size_t)B * R * sizeof(int));
    add_pitch_post(pl, B, sal, Tm, e->d_state, e->d_cp, pl.d_f0, true, (long long)shift, cache_start, read_start, R, pitchf, pitch, f0_in);
    *pitchf_out = pitchf; *pitch_out = pitch;
}

// hybrid f0 (f0_hybrid.hip.h): the one launch behind the members' builders.  A workgroup per stream: 1024 threads when it decodes RMVPE's
// salience (pitch_post_kernel's scan shape), else a thread per frame rounded up to a wave -- a latency item of at most B x 1024 values, nothing to fill the chip with
void launch_f0_hybrid(hipStream_t s, int B, int Tm, int n, int mode, const float *const *rows, int rm_at, const float *sal, int sal_cs, long long sal_bs, StreamState *st,
                      float *rm_f0, float *out)
{
    if (B < 1 || Tm < 1 || Tm > 1024 || n < 1 || n > HYBRID_MAX || (mode != 0 && mode != 1) || rm_at < -1 || rm_at >= n || !out) throw ShapeError("f0 hybrid: shape");
    HybridP hp{};
    for (int i = 0; i < n; i++) { if (i != rm_at && !rows[i]) throw ShapeError("f0 hybrid: a member row is missing"); hp.row[i] = i == rm_at ? nullptr : rows[i]; }
    if (rm_at >= 0 && (!sal || !st)) throw ShapeError("f0 hybrid: RMVPE's salience is missing");
    hp.n = n; hp.mode = mode; hp.Tm = Tm; hp.rm_at = rm_at;
    hp.sal = sal; hp.sal_cs = sal_cs; hp.sal_bs = sal_bs; hp.threshold = 0.03f;   // rvc.rs:122
    hp.st = st; hp.rm_f0 = rm_f0; hp.out = out;
    const int threads = rm_at >= 0 ? 1024 : (Tm + 63) / 64 * 64;
    hipLaunchKernelGGL(f0_hybrid_kernel, dim3(B), dim3(threads), 0, s, hp);
}

float *add_f0_hybrid(rvc_engine *e, Plan &pl, int B, int n, int mode, const float *const *rows, int rm_at, const T1 &sal)
{
    static_assert(HYBRID_MAX == HYBRID_MEMBERS_MAX, "the kernel's member count is the key's");
    const int Tm = pl.Tm;
    if (rm_at >= 0 && (sal.C != 360 || sal.T != Tm)) throw ShapeError("pitch decode: salience shape");
    float *out = pl.arena.floats((size_t)B * Tm);
    float *rm_f0 = rm_at >= 0 && pl.key.with_taps ? pl.arena.floats((size_t)B * Tm) : nullptr;
    struct Rows { const float *r[HYBRID_MAX]; } rr{};
    for (int i = 0; i < n && i < HYBRID_MAX; i++) rr.r[i] = rows[i];
    StreamState *st = e->d_state;
    pl.ops.push_back([=](hipStream_t s) { launch_f0_hybrid(s, B, Tm, n, mode, rr.r, rm_at, sal.p, sal.ld, sal.bs, st, rm_f0, out); });
    if (rm_f0) { T1 t; t.p = rm_f0; t.B = B; t.C = 1; t.T = Tm; t.ld = Tm; t.bs = Tm; add_tap(pl, "hy.rm_f0", t); }
    { T1 t; t.p = out; t.B = B; t.C = 1; t.T = Tm; t.ld = Tm; t.bs = Tm; add_tap(pl, "hy.f0", t); }
    return out;
}

}  // namespace rvc
