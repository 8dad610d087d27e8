// retrieval.hip -- flat-L2 index retrieval (rvc/src/rvc.rs:159 is a TODO in the reference; definition: SURVEY.md Appendix A.4, BASELINE configs 3-5):
// index load and its device-side layouts, the search section of an infer plan (flat, or IVF-probed: ivf.hip.h), the index entry points of the C ABI.
#include "engine_int.h"
#include "knn.hip.h"
#include "ivf.hip.h"
#include "kmeans.hip.h"
#include "index_build.hip.h"

namespace rvc {

// The retrieval section of an infer plan: queries from the ContentVec output, one-pass approximate scan (or one implicit GEMM for many streams),
// exact re-rank + blend into `phone`, exhaustive fallback for streams whose candidate set overflowed.
std::atomic<int> g_knn_test_lose{0};
// the plan's k picks the entry point of a retrieval kernel (bodies are template <int K>, K = 4 or 8; there is no run-time k inside the kernels)
#define KNN_KERNEL_FOR(stem, k) ((k) == KNN_KMAX ? stem##_k8_kernel : stem##_kernel)
static void build_exhaustive(rvc_engine *e, Plan &pl, int B, int C, int nq, int nblk, int first_raw, uint32_t skip_head, uint32_t R, int T, const T1 &phone, const T1 &cvo,
                             bool fast, int *d_overflow, float *d_q = nullptr, float *cand_d = nullptr, int *cand_i = nullptr);

// The IVF section, in place of the flat one for every stream count: two launches, no fallback list, nothing that can time out.
static void build_ivf(rvc_engine *e, Plan &pl, int B, int C, int nq, int first_raw, uint32_t skip_head, uint32_t R, int T, const T1 &phone, const T1 &cvo)
{
        if (!e->index.ivf.cent) throw ShapeError("no IVF structure attached to the index");
        const int nlist = (int)e->index.ivf.nlist, Q = B * nq;
        const int nprobe = std::min(pl.key.nprobe, nlist);
        float *D = pl.arena.floats((size_t)Q * nlist);
        int *scanned = (int *)pl.arena.alloc((size_t)Q * sizeof(int));
        pl.d_ivf_scanned = scanned; pl.ivf_queries = Q;
        snprintf(g_last_kernel, sizeof g_last_kernel, "knn_ivf");
        Plan *plp = &pl;
        {
            IvfCoarseP cp{}; cp.cent = e->index.ivf.cent.get(); cp.nlist = nlist; cp.dim = C; cp.cv = cvo.p; cp.cv_cs = cvo.ld; cp.cv_bs = cvo.bs; cp.first_raw = first_raw; cp.nq = nq; cp.Q = Q; cp.D = D;
            const size_t lds = (size_t)IVF_TQ * ivf_qs(C) * sizeof(float);
            if (lds > 128 * 1024) throw ShapeError("feature dimension too large for the retrieval kernel");
            dim3 grid((nlist + IVF_TC - 1) / IVF_TC, (Q + IVF_TQ - 1) / IVF_TQ);
            const double bytes = (double)nlist * C * sizeof(float);            // algorithmic bytes: the centroid table, once per launch
            pl.ops.push_back([=](hipStream_t s) {
                const ProfEvent *pe = plp->prof_slot(0, bytes, -1, "knn_ivf_coarse");
                if (pe) hipExtLaunchKernelGGL(ivf_coarse_kernel, grid, dim3(256), (uint32_t)lds, s, pe->a, pe->b, 0, cp);
                else hipLaunchKernelGGL(ivf_coarse_kernel, grid, dim3(256), lds, s, cp);
            });
        }
        {
            IvfScanP sp{}; sp.D = D; sp.nlist = nlist; sp.nprobe = nprobe; sp.offs = e->index.ivf.offs.get(); sp.perm = e->index.ivf.perm.get(); sp.index = e->index.rows.get(); sp.dim = C;
            sp.cv = cvo.p; sp.cv_cs = cvo.ld; sp.cv_bs = cvo.bs; sp.first_raw = first_raw; sp.nq = nq;
            sp.skip_head = (int)skip_head; sp.T = T; sp.R = (int)R; sp.rate = e->index_rate;
            sp.phone = phone.p; sp.ph_cs = phone.ld; sp.ph_bs = phone.bs; sp.out_idx = pl.d_knn_idx; sp.out_dist = pl.d_knn_dist; sp.scanned = scanned;
            const size_t lds = ((size_t)IVF_TILE + C) * sizeof(float);
            if (lds > 144 * 1024) throw ShapeError("feature dimension too large for the retrieval kernel");
            dim3 grid(nq, B);
            const auto scan_kernel = KNN_KERNEL_FOR(ivf_scan_blend, pl.key.knn_k);
            pl.ops.push_back([=](hipStream_t s) {
                const ProfEvent *pe = plp->prof_slot(0, 0, -1, "knn_ivf_scan");     // (bytes: the rows the probe sets held, read back by rvc_profile_last_knn)
                if (pe) hipExtLaunchKernelGGL(scan_kernel, grid, dim3(256), (uint32_t)lds, s, pe->a, pe->b, 0, sp);
                else hipLaunchKernelGGL(scan_kernel, grid, dim3(256), lds, s, sp);
            });
        }
}

void build_retrieval(rvc_engine *e, Plan &pl, int B, int T, int C, uint32_t skip_head, uint32_t R, const T1 &phone)
{
        if (e->index.dim != (size_t)C) throw std::runtime_error("index dimension does not match the feature dimension");
        // unique raw frames behind the sliced frames (Q2): first_raw .. last_raw
        const int first_raw = std::min((int)skip_head / 2, T - 1), last_raw = std::min((int)(skip_head + R - 1) / 2, T - 1);
        const int nq = last_raw - first_raw + 1;
        const int nblk = (int)((e->index.n + 255) / 256);
        const int K = pl.key.knn_k;
        if (K != KNN_K && K != KNN_KMAX) throw ShapeError("k must be 4 or 8");
        if (e->index.n < (size_t)K) throw ShapeError("index needs at least " + std::to_string(K) + " vectors");
        pl.d_knn_idx = (int *)pl.arena.alloc((size_t)B * R * K * sizeof(int));
        pl.d_knn_dist = pl.arena.floats((size_t)B * R * K);
        T1 cvo = pl.cv_out;
        if (pl.key.nprobe > 0) { build_ivf(e, pl, B, C, nq, first_raw, skip_head, R, T, phone, cvo); return; }
        // Stage A + B: approximate distances on the matrix cores in one pass over the index (HBM-bound), exact re-rank of a
        // provably sufficient candidate set.
        const bool fast = C % 16 == 0 && !test_opt("RVC_KNN_EXHAUSTIVE");
        // many streams: all queries against the index as ONE implicit GEMM (queries = weight operand in fragment order, transposed
        // index = activation operand, -|y|^2 / 2 as a per-column residual, scale -2): one pass over the index instead of one per 16
        // queries (64 streams x 11 queries: 44 passes, 3.5 ms -> one ~1 ms MFMA-bound launch).  Same approximate distances up to
        // fp32 summation order; the exact re-rank behind it is unchanged.
        const int Q = B * nq, Qpad = (Q + 127) / 128 * 128;
        // (the GEMM path addresses its operands with 32-bit byte / element offsets: the one-pass scan, whose strides are 64-bit, takes
        // indexes beyond that range)
        const bool gemm_fits = (size_t)C * e->index.n * sizeof(float) < ((size_t)1 << 31) && (size_t)Qpad * e->index.n < ((size_t)1 << 31);
        const bool gemm_scan = fast && Q >= 128 && gemm_fits && e->index.nhn && !test_opt("RVC_KNN_NO_GEMM");
        if (gemm_scan || !fast) ensure_index_transposed(e);
        if (fast && !gemm_scan) {
            // one stream / few streams: ONE launch per group of 16 queries (knn_scan_select_kernel: scan, select, exact re-rank, blend)
            // three workgroups per CU of the stream this runs on, all resident at once (the ContentVec branch is CU-masked at <= 4 streams)
            // (test hook RVC_KNN_WGS: another grid for the same result -- tiles per workgroup and the KNN_FUSED_MAXG cap without a 100 k-row index; tuning builds
            // also take it from the environment)
            const int wgs_opt = test_opt_int("RVC_KNN_WGS", 0);
            const unsigned knn_wgs = wgs_opt > 0 ? (unsigned)wgs_opt : 3u * (unsigned)e->cv_cus;
            const unsigned G = std::min(std::min((unsigned)((e->index.n + 63) / 64), std::max(knn_wgs / (unsigned)B, 64u)), (unsigned)KNN_FUSED_MAXG);
            const int ngroups = (nq + 15) / 16;
            snprintf(g_last_kernel, sizeof g_last_kernel, "knn_fused");
            unsigned long long *lists = (unsigned long long *)pl.arena.alloc((size_t)ngroups * B * 16 * G * K * sizeof(unsigned long long));
            unsigned *ticket = (unsigned *)pl.arena.alloc((size_t)ngroups * B * 2 * sizeof(unsigned));
            HIPCHK(hipMemset(ticket, 0, (size_t)ngroups * B * 2 * sizeof(unsigned)));
            pl.knn_ticket = ticket; pl.knn_ticket_bytes = (size_t)ngroups * B * 2 * sizeof(unsigned);
            for (int gi = 0; gi < ngroups; gi++) {
                const size_t lds = knn_fused_lds_floats(C, std::min(16, nq - gi * 16), (int)G, K) * sizeof(float);
                if (lds > 128 * 1024) throw ShapeError("feature dimension too large for the retrieval kernel");
                KnnFusedP fp{}; fp.indexF = e->index.rowsF.get(); fp.index = e->index.rows.get(); fp.ynorm = e->index.ynorm.get(); fp.n = (int)e->index.n; fp.dim = C;
                fp.cv = cvo.p; fp.cv_cs = cvo.ld; fp.cv_bs = cvo.bs; fp.first_raw = first_raw; fp.nq = nq; fp.q0 = gi * 16;
                fp.lists = lists + (size_t)gi * B * 16 * G * K; fp.ticket = ticket + (size_t)gi * B * 2;
                fp.skip_head = (int)skip_head; fp.T = T; fp.R = (int)R; fp.rate = e->index_rate;
                fp.phone = phone.p; fp.ph_cs = phone.ld; fp.ph_bs = phone.bs; fp.out_idx = pl.d_knn_idx; fp.out_dist = pl.d_knn_dist;
                fp.status = &e->d_state[0].status; fp.status_stride = (int)(sizeof(StreamState) / sizeof(int));
                fp.spin_limit = 1u << 22;
                dim3 grid(G, B);
                Plan *plp = &pl;
                const double scan_bytes = (double)e->index.n * C * sizeof(float) * B;     // algorithmic bytes: the index, read once per query group
                const auto fused_kernel = KNN_KERNEL_FOR(knn_scan_select, K);
                pl.ops.push_back([=](hipStream_t s) {
                    const ProfEvent *pe = plp->prof_slot(0, scan_bytes, -1, "knn_scan_select");
                    if (g_knn_test_lose.load(std::memory_order_relaxed)) {       // test hook (rvc_debug_option RVC_KNN_LOSE_TICKET): a hand-off that cannot complete
                        KnnFusedP f2 = fp; f2.test_lose = 1; f2.spin_limit = 1u << 12;
                        hipLaunchKernelGGL(fused_kernel, grid, dim3(256), lds, s, f2);
                    } else if (pe) hipExtLaunchKernelGGL(fused_kernel, grid, dim3(256), (uint32_t)lds, s, pe->a, pe->b, 0, fp);
                    else hipLaunchKernelGGL(fused_kernel, grid, dim3(256), lds, s, fp);
                });
            }
            // What the engine runs instead when a selector gave up (ST_KNN_TIMEOUT: a workgroup of the launch did not arrive in time, e.g. on a GPU
            // shared with another process): the exhaustive exact scan over the row-major index + merge + blend, built into a list of its own.
            // The chunk is then recomputed from `phone` on and the call returns RVC_OK (engine.hip recover_retrieval).
            if (!pl.key.bucket) {
                OpList main_ops = std::move(pl.ops);
                pl.ops = OpList();
                build_exhaustive(e, pl, B, C, nq, nblk, first_raw, skip_head, R, T, phone, cvo, false, nullptr);
                pl.knn_fallback = std::move(pl.ops.v);
                pl.ops = std::move(main_ops);
            }
            return;
        }
        // many streams (GEMM scan) or the exhaustive definition: explicit query rows, candidate lists per 256-vector block
        float *d_q = pl.arena.floats((size_t)B * nq * C);
        float *cand_d = pl.arena.floats((size_t)B * nq * nblk * K);
        int *cand_i = (int *)pl.arena.alloc((size_t)B * nq * nblk * K * sizeof(int));
        {
            dim3 grid((nq * C + 255) / 256, B);
            pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(knn_queries_kernel, grid, dim3(256), 0, s, cvo.p, cvo.ld, cvo.bs, C, first_raw, nq, d_q); });
        }
        // the exhaustive exact scan below runs for every stream (the definition), or only for streams whose candidate set overflowed
        int *d_overflow = (int *)pl.arena.alloc((size_t)B * sizeof(int));
        pl.d_knn_overflow = d_overflow;
        if (fast) {
            float *d_approx = pl.arena.floats((size_t)Qpad * e->index.n);
            float *d_qf = pl.arena.floats((size_t)Qpad * C);
            const int n_idx = (int)e->index.n;
            {
                dim3 grid(Qpad / 16, C / 16); int *ovf = d_overflow; const int nb = B;
                pl.ops.push_back([=](hipStream_t s) {
                    HIPCHK(hipMemsetAsync(ovf, 0, (size_t)nb * sizeof(int), s));
                    hipLaunchKernelGGL(knn_pack_queries_kernel, grid, dim3(64), 0, s, d_q, Q, C, d_qf);
                });
            }
            ConvW qw; qw.w = d_qf; qw.bias = nullptr; qw.M = Qpad; qw.K = C; qw.Kp = C; qw.Cin = C; qw.Cout = Qpad; qw.KW = 1; qw.groups = 1; qw.nphase = 1; qw.owns = false;
            T1 xi; xi.p = e->index.rowsT.get(); xi.B = 1; xi.C = C; xi.T = n_idx; xi.ld = n_idx; xi.halo = 0; xi.bs = (long long)C * n_idx;
            T1 ya; ya.p = d_approx; ya.B = 1; ya.C = Qpad; ya.T = n_idx; ya.ld = n_idx; ya.halo = 0; ya.bs = (long long)Qpad * n_idx;
            ConvOpts o; o.no_bias = true; o.res = e->index.nhn.get(); o.res_cs = 0; o.res_bs = 0; o.scale = -2.0f;
            add_conv1d(pl, qw, xi, ya, 1, 0, 1, o);
            KnnSelP sp{}; sp.approx = d_approx; sp.approx_bs = (long long)nq * e->index.n; sp.n = (int)e->index.n; sp.dim = C; sp.nq = nq;
            sp.index = e->index.rows.get(); sp.q = d_q; sp.q_bs = (long long)nq * C; sp.skip_head = (int)skip_head; sp.T = T; sp.R = (int)R; sp.first_raw = first_raw;
            sp.rate = e->index_rate; sp.phone = phone.p; sp.ph_cs = phone.ld; sp.ph_bs = phone.bs; sp.out_idx = pl.d_knn_idx; sp.out_dist = pl.d_knn_dist;
            sp.overflow = d_overflow;
            dim3 sgrid(nq, B);
            const size_t slds = (size_t)33 * (C + 4) * sizeof(float);
            if (slds > 128 * 1024) throw ShapeError("feature dimension too large for the retrieval kernel");
            const auto select_kernel = KNN_KERNEL_FOR(knn_select_blend, K);
            pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(select_kernel, sgrid, dim3(1024), slds, s, sp); });
        }
        build_exhaustive(e, pl, B, C, nq, nblk, first_raw, skip_head, R, T, phone, cvo, fast, d_overflow, d_q, cand_d, cand_i);
        snprintf(g_last_kernel, sizeof g_last_kernel, fast ? "knn_gemm" : "knn_exhaustive");      // (behind add_conv1d, which notes the GEMM's own family)
}

// The exhaustive exact scan (= the definition) + merge + blend.  d_q == nullptr: the section also gathers its own queries and owns its buffers.
static void build_exhaustive(rvc_engine *e, Plan &pl, int B, int C, int nq, int nblk, int first_raw, uint32_t skip_head, uint32_t R, int T, const T1 &phone, const T1 &cvo,
                             bool fast, int *d_overflow, float *d_q, float *cand_d, int *cand_i)
{
        const int K = pl.key.knn_k;
        if (!d_q) {
            d_q = pl.arena.floats((size_t)B * nq * C);
            cand_d = pl.arena.floats((size_t)B * nq * nblk * K);
            cand_i = (int *)pl.arena.alloc((size_t)B * nq * nblk * K * sizeof(int));
            dim3 grid((nq * C + 255) / 256, B);
            pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(knn_queries_kernel, grid, dim3(256), 0, s, cvo.p, cvo.ld, cvo.bs, C, first_raw, nq, d_q); });
        }
        for (int q0 = 0; q0 < nq; q0 += KNN_MAXQ) {
            const int qn = std::min(KNN_MAXQ, nq - q0);
            KnnP kp{}; kp.indexT = e->index.rowsT.get(); kp.index = e->index.rows.get(); kp.n = (int)e->index.n; kp.dim = C; kp.nblk = nblk;
            kp.v_stride = e->index.rowsT ? 1 : C; kp.d_stride = e->index.rowsT ? (long long)e->index.n : 1;
            // query sub-range: pointers offset so that [B][nq] strides stay those of the full arrays
            kp.q = d_q + (size_t)q0 * C; kp.nq = qn; kp.cand_d = cand_d + (size_t)q0 * nblk * K; kp.cand_i = cand_i + (size_t)q0 * nblk * K;
            kp.overflow = fast ? d_overflow : nullptr;
            const int nq_total = nq;
            dim3 grid(nblk, B);
            const auto scan_kernel = KNN_KERNEL_FOR(knn_scan, K);
            pl.ops.push_back([=](hipStream_t s) {
                KnnP k2 = kp; k2.q_bs = (long long)nq_total * C; k2.cand_bs = (long long)nq_total * nblk * K;
                hipLaunchKernelGGL(scan_kernel, grid, dim3(256), 0, s, k2);
            });
        }
        KnnBlendP bp{}; bp.cand_d = cand_d; bp.cand_i = cand_i; bp.nblk = nblk; bp.nq = nq; bp.index = e->index.rows.get(); bp.dim = C; bp.q = d_q;
        bp.skip_head = (int)skip_head; bp.T = T; bp.R = (int)R; bp.first_raw = first_raw; bp.rate = e->index_rate;
        bp.phone = phone.p; bp.ph_cs = phone.ld; bp.ph_bs = phone.bs; bp.out_idx = pl.d_knn_idx; bp.out_dist = pl.d_knn_dist;
        bp.overflow = fast ? d_overflow : nullptr;
        dim3 grid(nq, B);
        const auto merge_kernel = KNN_KERNEL_FOR(knn_merge_blend, K);
        pl.ops.push_back([=](hipStream_t s) { hipLaunchKernelGGL(merge_kernel, grid, dim3(256), 0, s, bp); });
}

// the engine's IVF structure goes: the search is flat again, and no plan that probed the lists stays
static void drop_index_ivf(rvc_engine *e)
{
    e->index.ivf = IvfLists(); e->index_nprobe = 0;
    drop_plans(e);
}

// The CSR of an assignment (list offsets + row permutation, rows ascending inside every list) by the counting sort of ivf.hip.h, queued on the engine's stream:
// what rvc_set_index_ivf attaches and what every update step of the k-means training walks.
static void ivf_build_csr(rvc_engine *e, const int *d_assign, size_t n, size_t nlist, int *d_counts, int *d_offs, int *d_perm)
{
    HIPCHK(hipMemsetAsync(d_counts, 0, nlist * sizeof(int), e->stream));
    hipLaunchKernelGGL(ivf_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, d_assign, (int)n, d_counts);
    hipLaunchKernelGGL(ivf_offsets_kernel, dim3(1), dim3(256), 0, e->stream, d_counts, (int)nlist, d_offs);
    hipLaunchKernelGGL(ivf_fill_kernel, dim3((unsigned)((nlist + 3) / 4)), dim3(256), 0, e->stream, d_assign, (int)n, (int)nlist, d_offs, d_perm);
}
// behind ivf_build_csr into l's arrays: check the offsets and note what rvc_index_ivf_info reports
static void ivf_note_lists(rvc_engine *e, IvfLists &l, size_t n, size_t nlist)
{
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    std::vector<int> offs(nlist + 1);
    HIPCHK(hipMemcpy(offs.data(), l.offs.get(), offs.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (offs[0] != 0 || (size_t)offs[nlist] != n) throw std::runtime_error("IVF structure: the device-side list offsets do not add up");
    l.nlist = nlist; l.longest = l.empty = 0;
    for (size_t i = 0; i < nlist; i++) {
        const size_t len = (size_t)(offs[i + 1] - offs[i]);
        l.longest = std::max(l.longest, len); l.empty += len == 0;
    }
}
// The one way a structure is attached, behind drop_index_ivf: the CSR of d_assign (d_counts: scratch of nlist ints) next to the centroids, built in a structure
// of its own that becomes the engine's only once its offsets have been accepted -- a failure leaves no structure and a flat search.  behind_csr: recorded
// behind the CSR's launches (the training's total time ends there).
static void attach_ivf(rvc_engine *e, DevBuf<float> cent, const int *d_assign, int *d_counts, size_t nlist, DevEvent *behind_csr = nullptr)
{
    const size_t n = e->index.n;
    IvfLists l;
    l.cent = std::move(cent);
    l.offs.alloc(nlist + 1); l.perm.alloc(n);
    ivf_build_csr(e, d_assign, n, nlist, d_counts, l.offs.get(), l.perm.get());
    if (behind_csr) behind_csr->record(e->stream);
    ivf_note_lists(e, l, n, nlist);
    e->index.ivf = std::move(l);
}

// ---- k-means training (kmeans.hip.h) ----
void KmeansWork::alloc(size_t n_, size_t dim_, size_t nlist_, const float *rows_)
{
    n = n_; dim = dim_; nlist = nlist_; rows = rows_;
    nwg = (int)((n + KM_TR - 1) / KM_TR); nparts = (int)((n + KM_RB - 1) / KM_RB);
    cent.alloc(nlist * dim); assign[0].alloc(n); assign[1].alloc(n); dist.alloc(n);
    moved_wg.alloc((size_t)nwg); part.alloc((size_t)nparts); obj.alloc(1); moved.alloc(1);
    counts.alloc(nlist); offs.alloc(nlist + 1); perm.alloc(n);
}
// one assign step against w.cent into w.assign[cur] / w.dist; prev: the assignment `moved` is counted against (null: every row counts).  Synchronises.
void kmeans_assign_step(rvc_engine *e, KmeansWork &w, const int *prev, int cur, double *objective, long long *moved)
{
    KmeansAssignP ap{}; ap.index = w.rows ? w.rows : e->index.rows.get(); ap.n = (int)w.n; ap.dim = (int)w.dim; ap.cent = w.cent.get(); ap.nlist = (int)w.nlist;
    ap.prev = prev; ap.assign = w.assign[cur].get(); ap.dist = w.dist.get(); ap.moved_wg = w.moved_wg.get();
    w.step.start(e->stream);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)w.nwg), dim3(256), 0, e->stream, ap);
    hipLaunchKernelGGL(kmeans_objective_kernel, dim3((unsigned)w.nparts), dim3(256), 0, e->stream, w.dist.get(), (int)w.n, w.part.get());
    hipLaunchKernelGGL(kmeans_objective_final_kernel, dim3(1), dim3(256), 0, e->stream, w.part.get(), w.nparts, w.moved_wg.get(), w.nwg, w.obj.get(), w.moved.get());
    w.step.stop(e->stream);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(objective, w.obj.get(), sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(moved, w.moved.get(), sizeof(long long), hipMemcpyDeviceToHost));
    w.ms_assign += w.step.ms();
}
// one update step: the CSR of w.assign[cur], then the means into w.cent in place (a list reads rows and writes its own centroid only).  Synchronises.
void kmeans_update_step(rvc_engine *e, KmeansWork &w, int cur)
{
    w.step.start(e->stream);
    ivf_build_csr(e, w.assign[cur].get(), w.n, w.nlist, w.counts.get(), w.offs.get(), w.perm.get());
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)w.nlist), dim3(256), 0, e->stream, w.rows ? w.rows : e->index.rows.get(), (int)w.dim, w.offs.get(), w.perm.get(), w.cent.get());
    w.step.stop(e->stream);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    w.ms_update += w.step.ms();
}

// upstream's rule for IVF<n>,Flat: min(floor(16 sqrt(n)), n / 39), clamped to [1, 65536]
static size_t kmeans_default_nlist(size_t n)
{
    size_t a = (size_t)std::floor(16.0 * std::sqrt((double)n));
    while (a > 0 && (double)a > 16.0 * std::sqrt((double)n)) a--;
    return std::min<size_t>(std::max<size_t>(std::min(a, n / 39), 1), IVF_MAX_NLIST);
}
// The seeded sample: the nlist rows with the smallest (h(seed, i), i), taken in ascending row number.  h is the 32-bit mixer "lowbias32"
// (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16) applied as h(seed, i) = m(i ^ m(seed + 0x9e3779b9)); tests/kmeans_ref.py restates it.
static inline uint32_t kmeans_mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
static std::vector<int32_t> kmeans_seeded_rows(size_t n, size_t nlist, uint32_t seed)
{
    const uint32_t ms = kmeans_mix(seed + 0x9e3779b9u);
    std::vector<uint64_t> key(n);
    for (size_t i = 0; i < n; i++) key[i] = ((uint64_t)kmeans_mix((uint32_t)i ^ ms) << 32) | (uint32_t)i;
    std::nth_element(key.begin(), key.begin() + (nlist - 1), key.end());
    std::vector<int32_t> rows(nlist);
    for (size_t j = 0; j < nlist; j++) rows[j] = (int32_t)(uint32_t)key[j];
    std::sort(rows.begin(), rows.end());
    return rows;
}

// Lloyd's iterations of one training over w's matrix: c_j = row init_rows[j], an assign step, then up to `iters` update steps each followed
// by an assign step, stopping behind an assign step that moved no row.  d_rows: device scratch of nlist ints.  -> the assignment buffer the last step wrote.
// rvc_train_index_ivf runs it over the loaded index, rvc_index_build_finish over the row store of a build.
static int kmeans_lloyd(rvc_engine *e, KmeansWork &w, const std::vector<int32_t> &init_rows, int *d_rows, int iters, std::vector<double> &obj, long long *moved, int *run)
{
    HIPCHK(hipMemcpyAsync(d_rows, init_rows.data(), w.nlist * sizeof(int), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(kmeans_gather_kernel, dim3((unsigned)w.nlist), dim3(256), 0, e->stream, w.rows ? w.rows : e->index.rows.get(), (int)w.dim, d_rows, w.cent.get());
    obj.assign(1, 0.0);
    int cur = 0;
    *run = 0; *moved = 0;
    kmeans_assign_step(e, w, nullptr, cur, &obj[0], moved);
    while (*run < iters && *moved != 0) {
        kmeans_update_step(e, w, cur);
        double j = 0.0;
        kmeans_assign_step(e, w, w.assign[cur].get(), cur ^ 1, &j, moved);
        obj.push_back(j); cur ^= 1; (*run)++;
    }
    return cur;
}

// no index: the matrix, every layout and the IVF structure go, the search is flat, and no plan of the old index stays
static void drop_index(rvc_engine *e)
{
    e->index = RetrievalIndex(); e->index_nprobe = 0;
    drop_plans(e);
}

// The one way a matrix becomes the engine's index: rvc_load_index[_device], rvc_index_build_finish and rvc_index_broadcast all end here.  Everything the
// retrieval kernels need besides the row-major matrix is built ON THE DEVICE from the copy that is already in HBM (uploaded once, handed over by a build, or
// delivered by the RCCL broadcast): the MFMA-fragment-order copy for the one-pass approximate scan and the vector norms.  No host round trip (round 2 copied
// the 307 MB matrix back to the host, repacked it in a single-threaded loop and uploaded two more copies: seconds per rank behind a 2 ms broadcast).  The
// transposed copy is NOT built here: see ensure_index_transposed.
// The contract: whatever refuses a call before it gets here (n < index_k, dim < 1, a finish refused by its checks, a broadcast refused in its agreement round)
// leaves the old index in place.  From the first line of this function on the engine has either the new index complete -- flat search, no IVF structure, no
// plan of the old one -- or, when a step throws, no index and no stale plans; never a mixture.  index_k and index_rate survive either way.
void install_index(rvc_engine *e, DevBuf<float> rows, size_t n, size_t dim)
{
    drop_index(e);
    RetrievalIndex &ix = e->index;
    try {
        ix.rows = std::move(rows);
        DevTimer prep; prep.start(e->stream);
        if (dim % 16 == 0) {
            const long long nt = ((long long)n + 15) / 16, nc = (long long)dim / 16, total4 = nt * nc * 64;
            ix.rowsF.alloc((size_t)total4 * 4);
            hipLaunchKernelGGL(knn_pack_index_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, e->stream, ix.rows.get(), (long long)n, (int)dim, ix.rowsF.get(), total4);
        }
        ix.ynorm.alloc(n); ix.nhn.alloc(n);
        hipLaunchKernelGGL(knn_norms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, ix.rows.get(), (int)n, (int)dim, ix.ynorm.get(), ix.nhn.get());
        prep.stop(e->stream);
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        ix.prep_ms = prep.ms();
        ix.n = n; ix.dim = dim;
    } catch (...) { ix = RetrievalIndex(); throw; }
}

// [dim][n] copy of the index, built by a device transpose the first time a plan needs it: the many-stream distance GEMM (the index is
// its activation operand) and the forced / non-MFMA exhaustive scan.  A single stream never builds it (HBM then holds the index twice:
// row-major for the exact re-rank and the blend, fragment order for the scan); its degenerate-data fallback walks the row-major copy.
void ensure_index_transposed(rvc_engine *e)
{
    RetrievalIndex &ix = e->index;
    if (ix.rowsT || !ix.rows) return;
    ix.rowsT.alloc(ix.n * ix.dim);
    dim3 grid((unsigned)((ix.n + 31) / 32), (unsigned)((ix.dim + 31) / 32));
    hipLaunchKernelGGL(knn_transpose_kernel, grid, dim3(256), 0, e->stream, ix.rows.get(), (long long)ix.n, (int)ix.dim, ix.rowsT.get());
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
}

// ---- the index builder (index_build.hip.h) ----
void IndexBuild::alloc(size_t dim_, size_t capacity_)
{
    dim = dim_; capacity = capacity_;
    store.alloc(capacity * dim);
    d_cnt.alloc(2);
    HIPCHK(hipMemset(d_cnt.get(), 0, 2 * sizeof(int)));
}
// room for `need` rows; `upper` = an upper bound of the rows the store holds (the device's own count is not known between the windows of an add)
void index_build_reserve(rvc_engine *e, IndexBuild &b, size_t upper, size_t need)
{
    if (need > (size_t)0x7fffffff) throw ShapeError("index build: more than 2^31 - 1 rows");
    if (need <= b.capacity) return;
    const size_t cap = std::max(2 * b.capacity, need);
    DevBuf<float> grown; grown.alloc(cap * b.dim);
    if (upper) HIPCHK(hipMemcpyAsync(grown.get(), b.store.get(), upper * b.dim * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    b.retired.emplace_back((char *)b.store.release());      // (the copy above, and appends queued before it, still read it)
    b.store = std::move(grown); b.capacity = cap;
}
void index_build_append(rvc_engine *e, IndexBuild &b, const float *cv, int C, int T, int ld)
{
    if ((size_t)C != b.dim || T < 1 || ld < T) throw ShapeError("index build: the window's feature matrix does not match the store");
    if ((size_t)T > b.bad_cap) {
        if (b.d_bad) b.retired.emplace_back((char *)b.d_bad.release());
        b.bad_cap = 0;
        const size_t cap = std::max((size_t)T, (size_t)1024);
        b.d_bad.alloc(cap);
        b.bad_cap = cap;
        HIPCHK(hipMemsetAsync(b.d_bad.get(), 0, cap * sizeof(int), e->stream));
    }
    IndexAppendP p{}; p.cv = cv; p.C = C; p.T = T; p.ld = ld; p.rows = b.store.get(); p.capacity = (long long)b.capacity; p.cnt = b.d_cnt.get(); p.bad = b.d_bad.get();
    dim3 grid((unsigned)((T + IB_TILE - 1) / IB_TILE), (unsigned)((C + IB_TILE - 1) / IB_TILE));
    hipLaunchKernelGGL(index_append_kernel, grid, dim3(256), 0, e->stream, p);
    hipLaunchKernelGGL(index_compact_kernel, dim3(1), dim3(256), 0, e->stream, b.store.get(), C, (long long)b.capacity, b.d_bad.get(), T, b.d_cnt.get());
}
void index_build_abort(rvc_engine *e)
{
    if (!e->ib) return;
    (void)hipDeviceSynchronize();
    delete e->ib;
    e->ib = nullptr;
}
static hipEvent_t ib_event(IndexBuild &b, size_t i)
{
    if (b.ev.size() <= i) b.ev.resize(i + 1);
    return b.ev[i].get();
}
// One recording: consecutive windows, the tail at its own length when ContentVec yields a frame for it.  Per run: the samples into the plan's input, the plan,
// the append.  One synchronisation and one read of the device counters at the end.
static rvc_status index_build_add(rvc_engine *e, const void *pcm, size_t n, bool on_device, size_t *rows_added)
{
    if (rows_added) *rows_added = 0;
    if (!e->ib) throw ShapeError("index build: no build is open (rvc_index_build_begin)");
    if (!e->cv) { e->err = "index build: ContentVec is not loaded"; return RVC_CONTENTVEC_NOT_LOADED; }
    if (!pcm && n) throw ShapeError("index build: null recording");
    IndexBuild &b = *e->ib;
    size_t upper = b.rows, runs = 0;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    try {
        for (size_t start = 0; start < n; start += b.window) {
            const size_t len = std::min(b.window, n - start);
            const int T = e->cv->out_frames(len);
            if (T < 1) break;                                    // (the tail, shorter than ContentVec's receptive field: dropped)
            Plan *pl = hubert_plan(e, len);
            if ((size_t)pl->C != b.dim || pl->T != T) throw ShapeError("index build: ContentVec changed while the build was open");
            HIPCHK(hipMemcpyAsync(pl->d_in, (const float *)pcm + start, len * sizeof(float), kind, e->stream));
            HIPCHK(hipEventRecord(ib_event(b, 3 * runs), e->stream));
            run_hubert_plan(e, *pl);
            HIPCHK(hipEventRecord(ib_event(b, 3 * runs + 1), e->stream));
            index_build_reserve(e, b, upper, upper + (size_t)T);
            index_build_append(e, b, pl->cv_out.p, pl->C, T, pl->cv_out.ld);
            HIPCHK(hipEventRecord(ib_event(b, 3 * runs + 2), e->stream));
            upper += (size_t)T; runs++;
        }
    } catch (...) {
        // what was queued still runs: bring the host's view up to date before the error leaves
        int cnt[2] = {0, 0};
        if (hipStreamSynchronize(e->stream) == hipSuccess && hipMemcpy(cnt, b.d_cnt.get(), sizeof cnt, hipMemcpyDeviceToHost) == hipSuccess) { b.rows = (size_t)cnt[0]; b.dropped = (size_t)cnt[1]; }
        b.retired.clear();
        throw;
    }
    int cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt, b.d_cnt.get(), sizeof cnt, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    b.retired.clear();
    for (size_t w = 0; w < runs; w++) {
        float a = 0.f, c = 0.f;
        HIPCHK(hipEventElapsedTime(&a, b.ev[3 * w].get(), b.ev[3 * w + 1].get()));
        HIPCHK(hipEventElapsedTime(&c, b.ev[3 * w + 1].get(), b.ev[3 * w + 2].get()));
        b.ms[0] += a; b.ms[1] += c;
    }
    if ((size_t)cnt[0] + (size_t)(cnt[1] - (int)b.dropped) != upper) throw std::runtime_error("index build: the device-side row count does not add up");
    if (rows_added) *rows_added = (size_t)cnt[0] - b.rows;
    b.rows = (size_t)cnt[0]; b.dropped = (size_t)cnt[1]; b.windows += runs;
    return RVC_OK;
}

void retrieval_kernel_attrs()
{
    HIPCHK(hipFuncSetAttribute((const void *)knn_select_blend_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));   // + ~5 KB static
    HIPCHK(hipFuncSetAttribute((const void *)knn_select_blend_k8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)knn_scan_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)knn_scan_select_k8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));   // + ~5 KB static
    HIPCHK(hipFuncSetAttribute((const void *)ivf_coarse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));         // + 16 KB static
    HIPCHK(hipFuncSetAttribute((const void *)ivf_scan_blend_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));     // + ~2 KB static
    HIPCHK(hipFuncSetAttribute((const void *)ivf_scan_blend_k8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
}

}  // namespace rvc

using namespace rvc;
extern "C" {

// rvc_load_index / rvc_load_index_device: the old index goes before the new matrix is allocated (HBM never holds two matrices), so a failure behind the
// argument checks leaves no index
static rvc_status load_index(rvc_engine *e, const void *vectors, size_t n, size_t dim, hipMemcpyKind kind)
{
    return guarded(e, [&]() {
        if (n < (size_t)e->index_k || dim < 1) throw ShapeError("index needs at least " + std::to_string(e->index_k) + " vectors");
        HIPCHK(hipDeviceSynchronize());
        drop_index(e);
        DevBuf<float> rows; rows.alloc(n * dim);
        HIPCHK(hipMemcpy(rows.get(), vectors, n * dim * sizeof(float), kind));
        install_index(e, std::move(rows), n, dim);
        return RVC_OK;
    });
}

rvc_status rvc_load_index(rvc_engine *e, const float *vectors, size_t n, size_t dim) { return load_index(e, vectors, n, dim, hipMemcpyHostToDevice); }

rvc_status rvc_load_index_device(rvc_engine *e, const void *d_vectors, size_t n, size_t dim) { return load_index(e, d_vectors, n, dim, hipMemcpyDeviceToDevice); }

void *rvc_index_device_ptr(rvc_engine *e, size_t *bytes)
{
    if (!e || !e->index.rows) { if (bytes) *bytes = 0; return nullptr; }
    if (bytes) *bytes = e->index.n * e->index.dim * sizeof(float);
    return e->index.rows.get();
}

rvc_status rvc_get_knn(rvc_engine *e, int32_t *idx, float *dist, size_t cap_rows, size_t *rows)
{
    return guarded(e, [&]() {
        Plan *pl = e->last_plan;
        // (after rvc_infer_batch_g the last plan is one geometry bucket's, in bucket-local stream order: no rows are reported for such a call)
        if (!pl || !pl->key.with_index || !e->last_knn_rows) { if (rows) *rows = 0; return RVC_OK; }
        // stream 0's return_length rows always; the further streams' rows (stream-major) as far as the caller's capacity holds whole streams
        if (cap_rows < pl->key.R) { if (rows) *rows = pl->key.R; return RVC_SHAPE; }
        const size_t r = pl->key.R * std::min((size_t)pl->key.B, cap_rows / pl->key.R);
        if (rows) *rows = r;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(idx, pl->d_knn_idx, r * pl->key.knn_k * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dist, pl->d_knn_dist, r * pl->key.knn_k * sizeof(float), hipMemcpyDeviceToHost));
        return RVC_OK;
    });
}

// Attach an IVF structure to the loaded index: centroids and assignment are copied, validated on the host, and the CSR (list offsets + row permutation, rows
// ascending inside every list) is built on the device by a counting sort.  The matrix itself is not copied: the scan gathers whole rows by id.
rvc_status rvc_set_index_ivf(rvc_engine *e, const float *centroids, size_t nlist, size_t dim, const int32_t *assign, size_t n)
{
    return guarded(e, [&]() {
        if (!e->index.rows) throw ShapeError("no index loaded");
        if (!centroids || !assign) throw ShapeError("IVF structure: null centroids or assignment");
        if (dim != e->index.dim || n != e->index.n) throw ShapeError("IVF structure does not match the loaded index (dim or n)");
        if (nlist < 1 || nlist > IVF_MAX_NLIST) throw ShapeError("IVF structure: nlist must be in [1, 65536]");
        for (size_t i = 0; i < n; i++) if (assign[i] < 0 || (size_t)assign[i] >= nlist) throw ShapeError("IVF structure: an assignment is outside [0, nlist)");
        for (size_t i = 0; i < nlist * dim; i++) if (!std::isfinite(centroids[i])) throw ShapeError("IVF structure: a centroid is not finite");
        HIPCHK(hipDeviceSynchronize());
        drop_index_ivf(e);
        DevBuf<float> cent; DevBuf<int> d_assign, d_counts;
        cent.alloc(nlist * dim); d_assign.alloc(n); d_counts.alloc(nlist);
        HIPCHK(hipMemcpy(cent.get(), centroids, nlist * dim * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_assign.get(), assign, n * sizeof(int), hipMemcpyHostToDevice));
        attach_ivf(e, std::move(cent), d_assign.get(), d_counts.get(), nlist);
        return RVC_OK;
    });
}

// k-means over the loaded index (kmeans.hip.h), then the attachment rvc_set_index_ivf makes.  Everything that can refuse the call is decided before the structure
// the engine has is dropped; a failure behind that point leaves no structure and a flat search.
rvc_status rvc_train_index_ivf(rvc_engine *e, size_t nlist, int iters, const int32_t *init_rows, uint32_t seed)
{
    return guarded(e, [&]() {
        if (!e->index.rows) throw ShapeError("no index loaded");
        const size_t n = e->index.n, dim = e->index.dim;
        if (nlist == 0) nlist = kmeans_default_nlist(n);
        if (nlist > n || nlist > IVF_MAX_NLIST) throw ShapeError("k-means: nlist must be at most the number of rows and at most 65536");
        if (iters < 0 || iters > 100) throw ShapeError("k-means: iters must be in [0, 100]");
        std::vector<int32_t> rows;
        if (init_rows) {
            rows.assign(init_rows, init_rows + nlist);
            std::vector<char> seen(n, 0);
            for (size_t j = 0; j < nlist; j++) {
                if (rows[j] < 0 || (size_t)rows[j] >= n) throw ShapeError("k-means: initial row " + std::to_string(j) + " is outside the index");
                if (seen[rows[j]]) throw ShapeError("k-means: row " + std::to_string(rows[j]) + " appears twice among the initial rows");
                seen[rows[j]] = 1;
            }
        } else rows = kmeans_seeded_rows(n, nlist, seed);
        HIPCHK(hipDeviceSynchronize());
        DevBuf<int> d_rows;                                                  // (also the word the non-finite search answers in)
        d_rows.alloc(std::max(nlist, (size_t)1));
        int first = 0x7fffffff;
        HIPCHK(hipMemcpy(d_rows.get(), &first, sizeof(int), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(kmeans_nonfinite_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, e->index.rows.get(), e->index.ynorm.get(), (int)n, (int)dim, d_rows.get());
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(&first, d_rows.get(), sizeof(int), hipMemcpyDeviceToHost));
        if (first != 0x7fffffff) throw ShapeError("k-means: row " + std::to_string(first) + " of the index holds a NaN or an Inf");
        // ---- from here on the old structure is gone ----
        drop_index_ivf(e);
        e->km_valid = false;
        KmeansWork w;
        w.alloc(n, dim, nlist);
        DevTimer total; total.start(e->stream);
        std::vector<double> obj; long long moved = 0; int run = 0;
        const int cur = kmeans_lloyd(e, w, rows, d_rows.get(), iters, obj, &moved, &run);
        // attach: the centroids as they are, the CSR of the last assign step
        attach_ivf(e, std::move(w.cent), w.assign[cur].get(), w.counts.get(), nlist, &total.b);
        e->km_iters_run = run; e->km_moved_last = (size_t)moved; e->km_obj = obj;
        e->km_ms[0] = w.ms_assign; e->km_ms[1] = w.ms_update; e->km_ms[2] = total.ms();
        e->km_valid = true;
        return RVC_OK;
    });
}

rvc_status rvc_index_ivf_train_info(rvc_engine *e, int *iters_run, size_t *moved_last, double *objective, size_t cap, size_t *n_obj, double ms[3])
{
    return guarded(e, [&]() {
        if (!e->km_valid) throw ShapeError("no k-means training has completed on this engine");
        if (iters_run) *iters_run = e->km_iters_run;
        if (moved_last) *moved_last = e->km_moved_last;
        if (n_obj) *n_obj = e->km_obj.size();
        if (objective) for (size_t i = 0; i < std::min(cap, e->km_obj.size()); i++) objective[i] = e->km_obj[i];
        if (ms) for (int i = 0; i < 3; i++) ms[i] = e->km_ms[i];
        return RVC_OK;
    });
}

// the attached structure, trained or set: the centroids as stored, the assignment rebuilt from the CSR
rvc_status rvc_get_index_ivf(rvc_engine *e, float *centroids, size_t cap_centroid_floats, int32_t *assign, size_t cap_rows)
{
    return guarded(e, [&]() {
        if (!e->index.ivf.cent) throw ShapeError("no IVF structure attached to the index");
        const size_t nlist = e->index.ivf.nlist, n = e->index.n, dim = e->index.dim;
        if (!centroids || !assign || cap_centroid_floats < nlist * dim || cap_rows < n) throw ShapeError("IVF structure: the caller's arrays are too short");
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(centroids, e->index.ivf.cent.get(), nlist * dim * sizeof(float), hipMemcpyDeviceToHost));
        std::vector<int> offs(nlist + 1), perm(n);
        HIPCHK(hipMemcpy(offs.data(), e->index.ivf.offs.get(), offs.size() * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(perm.data(), e->index.ivf.perm.get(), n * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t l = 0; l < nlist; l++)
            for (int q = offs[l]; q < offs[l + 1]; q++) assign[perm[q]] = (int32_t)l;
        return RVC_OK;
    });
}

rvc_status rvc_set_index_nprobe(rvc_engine *e, int nprobe)
{
    return guarded(e, [&]() {
        if (!e->index.rows) throw ShapeError("no index loaded");
        if (nprobe < 0 || nprobe > IVF_MAX_NPROBE) throw ShapeError("nprobe must be in [0, 64]");
        if (nprobe >= 1 && !e->index.ivf.cent) throw ShapeError("nprobe >= 1 needs an IVF structure (rvc_set_index_ivf)");
        e->index_nprobe = nprobe >= 1 ? (int)std::min((size_t)nprobe, e->index.ivf.nlist) : 0;
        return RVC_OK;
    });
}

int rvc_index_nprobe(rvc_engine *e) { return e ? e->index_nprobe : 0; }

// Neighbours per query: 4 (the default) or upstream's 8.  A preference of the caller: it outlives index loads, broadcasts and IVF structures, and the plans
// keyed on it stay in the cache (changing it back finds them).
rvc_status rvc_set_index_k(rvc_engine *e, int k)
{
    return guarded(e, [&]() {
        if (k != KNN_K && k != KNN_KMAX) throw ShapeError("k must be 4 or 8");
        if (e->index.rows && e->index.n < (size_t)k) throw ShapeError("the loaded index has fewer than " + std::to_string(k) + " vectors");
        e->index_k = k;
        return RVC_OK;
    });
}

int rvc_index_k(rvc_engine *e) { return e ? e->index_k : KNN_K; }

rvc_status rvc_index_ivf_info(rvc_engine *e, size_t *nlist, size_t *longest_list, size_t *empty_lists)
{
    return guarded(e, [&]() {
        if (!e->index.ivf.cent) throw ShapeError("no IVF structure attached to the index");
        if (nlist) *nlist = e->index.ivf.nlist;
        if (longest_list) *longest_list = e->index.ivf.longest;
        if (empty_lists) *empty_lists = e->index.ivf.empty;
        return RVC_OK;
    });
}

// ---- the index builder: ContentVec frames of a voice's recordings into a row store on the device, then installed as the engine's index ----
rvc_status rvc_index_build_begin(rvc_engine *e, size_t window, size_t capacity_hint)
{
    return guarded(e, [&]() {
        if (!e->cv) { e->err = "index build: ContentVec is not loaded"; return RVC_CONTENTVEC_NOT_LOADED; }
        if (e->ib) throw ShapeError("index build: a build is already open (finish or abort it first)");
        if (window == 0) window = 48000;
        if (capacity_hint == 0) capacity_hint = 4096;
        if (capacity_hint > (size_t)0x7fffffff) throw ShapeError("index build: more than 2^31 - 1 rows");
        Plan *pl = hubert_plan(e, window);                      // ("input too short for ContentVec": RVC_SHAPE)
        std::unique_ptr<IndexBuild> b(new IndexBuild());
        b->window = window;
        b->alloc((size_t)pl->C, capacity_hint);
        e->ib = b.release();
        return RVC_OK;
    });
}

rvc_status rvc_index_build_add(rvc_engine *e, const float *pcm16k, size_t n, size_t *rows_added)
{
    return guarded(e, [&]() { return index_build_add(e, pcm16k, n, false, rows_added); });
}

rvc_status rvc_index_build_add_device(rvc_engine *e, const void *d_pcm16k, size_t n, size_t *rows_added)
{
    return guarded(e, [&]() { return index_build_add(e, d_pcm16k, n, true, rows_added); });
}

rvc_status rvc_index_build_info(rvc_engine *e, size_t *rows, size_t *capacity, size_t *windows, size_t *dropped_nonfinite, double ms[3])
{
    return guarded(e, [&]() {
        if (!e->ib) throw ShapeError("index build: no build is open (rvc_index_build_begin)");
        if (rows) *rows = e->ib->rows;
        if (capacity) *capacity = e->ib->capacity;
        if (windows) *windows = e->ib->windows;
        if (dropped_nonfinite) *dropped_nonfinite = e->ib->dropped;
        if (ms) for (int i = 0; i < 3; i++) ms[i] = e->ib->ms[i];
        return RVC_OK;
    });
}

// Everything that can refuse the call is decided before anything changes: a refused finish leaves the build open and the engine's index in place.
rvc_status rvc_index_build_finish(rvc_engine *e, size_t max_rows, size_t reduce_to, int iters, uint32_t seed)
{
    return guarded(e, [&]() {
        if (!e->ib) throw ShapeError("index build: no build is open (rvc_index_build_begin)");
        IndexBuild &b = *e->ib;
        if (max_rows == 0) max_rows = 200000;                   // upstream's rule: above 200 000 rows ...
        if (reduce_to == 0) reduce_to = 10000;                  // ... 10 000 k-means centres
        const size_t rows = b.rows, dim = b.dim;
        const bool reduce = rows > max_rows;
        if (reduce && reduce_to > rows) throw ShapeError("index build: reduce_to is above the " + std::to_string(rows) + " rows the build holds");
        if (reduce && reduce_to > IVF_MAX_NLIST) throw ShapeError("index build: reduce_to must be at most 65536");
        if (reduce && (iters < 0 || iters > 100)) throw ShapeError("k-means: iters must be in [0, 100]");
        const size_t n = reduce ? reduce_to : rows;
        if (n < (size_t)e->index_k) throw ShapeError("index needs at least " + std::to_string(e->index_k) + " vectors (the build would install " + std::to_string(n) + ")");
        HIPCHK(hipDeviceSynchronize());
        DevBuf<float> installed;
        if (reduce) {
            // the trainer of rvc_train_index_ivf on the store's pointer: same seeded sample, same steps, same early stop.  The centroid table is an allocation
            // of exactly [reduce_to][dim] in centre order: it becomes the index as it is (no copy into the store's head), and the store is freed.
            const std::vector<int32_t> init = kmeans_seeded_rows(rows, reduce_to, seed);
            DevBuf<int> d_rows; d_rows.alloc(reduce_to);
            KmeansWork w;
            w.alloc(rows, dim, reduce_to, b.store.get());
            std::vector<double> obj; long long moved = 0; int run = 0;
            (void)kmeans_lloyd(e, w, init, d_rows.get(), iters, obj, &moved, &run);
            b.ms[2] += w.ms_assign + w.ms_update;
            installed = std::move(w.cent);
        } else if (b.capacity - rows > rows / 4) {
            // the store was grown by doubling: more than a quarter of slack is not worth keeping for the index's life
            installed.alloc(rows * dim);
            HIPCHK(hipMemcpy(installed.get(), b.store.get(), rows * dim * sizeof(float), hipMemcpyDeviceToDevice));
        } else {
            installed = std::move(b.store);                     // handed over without a copy
        }
        // installed as rvc_load_index_device installs a matrix
        delete e->ib; e->ib = nullptr;
        install_index(e, std::move(installed), n, dim);
        return RVC_OK;
    });
}

void rvc_index_build_abort(rvc_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    index_build_abort(e);
}

// chunks whose retrieval was recomputed through the exhaustive launches after a hand-off time-out of the one-launch form (they returned RVC_OK)
long long rvc_retrieval_recoveries(rvc_engine *e) { return e ? e->knn_recoveries : 0; }

}  // extern "C"
