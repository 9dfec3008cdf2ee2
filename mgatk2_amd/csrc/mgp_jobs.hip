// mgp_jobs.hip — the host drivers of everything that reads a finished run's rows, and
// their C-ABI entry points (include/mgpileup.h): the txt and HDF5 writers (kernels in
// mgp_txtgz.hip), the variant statistics (mgp_variants.hip) and the coverage QC passes
// (mgp_qc.hip), and the pseudobulk counts per cell group (mgp_groups.hip). Each job has two
// forms: *_run on a context's last run, whose rows it gets
// through run_rows (mgp_jobs.h: the context itself is opaque here), and the detached
// *_rows form on u32 rows of the caller's (on_rows). The clustering of the heteroplasmy
// matrix (mgp_cluster.hip) reads no rows and needs no context: mgp_pair_dist / mgp_hclust*;
// nor do the cells' neighbour graphs (mgp_graph.hip): mgp_knn / mgp_snn; nor the communities of
// such a graph (mgp_louvain.hip): mgp_louvain; nor the matrix's principal components
// (mgp_pca.hip): mgp_pca / mgp_sym_eig.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/mgpileup.h"
#include "mgp_cluster.h"
#include "mgp_graph.h"
#include "mgp_groups.h"
#include "mgp_host.h"
#include "mgp_jobs.h"
#include "mgp_louvain.h"
#include "mgp_pca.h"
#include "mgp_qc.h"
#include "mgp_rank.h"
#include "mgp_txtgz.h"
#include "mgp_variants.h"

using namespace mgp;

// mgp_txt_gz: the device txt writer's buffers (mgp_txtgz.hip), kept for the next call
struct TxtState {
    DevBuf cells, names, name_off, sizes, nlines, offs, text, tok, lines, out, member_bytes, crc_shift, dst_off, packed;
    DevBuf prof;  // MGP_TXT_PROF
    DevBuf seg, crc;
    bool shift_ready = false;
    int64_t n = 0;
    uint64_t total = 0;
};

// mgp_h5_tiles: the HDF5 chunk deflate's buffers (mgp_txtgz.hip), kept for the next call
struct H5State {
    DevBuf coc, raw, tok, out, out_off, chunk_bytes, dst_off, packed, sums, prof;
    uint64_t total = 0;
};

// mgp_variant_* / mgp_allele_freq_*: the variant reductions' buffers (mgp_variants.hip)
struct VarState {
    DevBuf cells, acc, part, f64, mu, pos, base, bad, out;
};

// mgp_group_moments_run / mgp_rows_group_moments: the grouped sweep's buffers (mgp_groups.hip)
struct GroupState {
    DevBuf cells, items, acc, bad;
    void release() {
        cells.release(), items.release(), acc.release(), bad.release();
    }
};

// mgp_cell_coverage_* / mgp_position_*: the coverage QC passes' buffers (mgp_qc.hip)
struct QcState {
    DevBuf cells, out64, out32, bad, in32, hist;
};

// mgp_pair_dist / mgp_hclust*: the clustering's buffers (mgp_cluster.hip), a call's own
struct ClusterState {
    DevBuf x, dist, bad, nn, dnn, act, list, si, sj, sh;
};

// mgp_knn / mgp_snn: the neighbour graphs' buffers (mgp_graph.hip), a call's own
struct GraphState {
    DevBuf x, bad, part_dist, part_idx, out_dist, out_idx;                 // mgp_knn
    DevBuf idx, sets, deg, off, cur, rev, cnt, eoff, ei, ej, es;  // mgp_snn
};

// mgp_rank_sums: the rank sums' buffers (mgp_rank.hip), a call's own
struct RankState {
    DevBuf x, group, keys, pay, r2, pos, ties, bad;
};

// mgp_pca / mgp_sym_eig: the principal components' buffers (mgp_pca.hip), a call's own
struct PcaState {
    DevBuf x, z, part, mean, var, sd, covp, cov, scores, bad;  // mgp_pca
    DevBuf a[2], v[2], vec, perm, maxabs, flag;                // the eigensolver: A and V ping-ponged
};

// mgp_louvain: the community detection's buffers (mgp_louvain.hip), a call's own
struct LouvainState {
    DevBuf ei, ej, wq, res, deg, cur, tkeys, tvals;                // the edge list, the results' words, the tables
    DevBuf off[2], nbr[2], src[2], w[2], d[2], self[2];            // this level's graph and the next one's
    DevBuf c, next, tot, tot_next, list_mid, list_long, counts;    // a level's labels, totals and row lists
    DevBuf flag, ren, cap, slot, map;                              // the aggregation
};

struct RowJobs {
    TxtState txt;
    H5State h5;
    VarState var;
    QcState qc;
    GroupState grp;
};
RowJobs* row_jobs_new() { return new RowJobs(); }
void row_jobs_free(RowJobs* jobs) { delete jobs; }

// The detached (*_rows) forms: the planes of the caller's u32 rows that the entry point
// needs are uploaded and `job(state, stream, rows, tn5)` runs on them with a fresh State,
// on a stream of the call's own; everything is freed once that stream is idle. A needed
// plane that is null (with rows to read) is refused before any device call.
enum { PL_COUNTS = 1, PL_TN5 = 2, PL_DEPTH = 4 };
struct HostRows {
    const uint32_t *counts, *tn5, *depth;  // [n_rows][mito_len] x 8, 2, 1 words; null where not needed
    int32_t n_rows, mito_len;
};
template <class State, class Job>
static int on_rows(int device, const char* who, int need, const HostRows& h, Job&& job) {
    const uint32_t* src[3] = {h.counts, h.tn5, h.depth};
    const size_t row_bytes[3] = {32, 8, 4};  // per position
    const int32_t n_rows = h.n_rows, mito_len = h.mito_len;
    bool ok = n_rows >= 0 && mito_len > 0;
    for (int k = 0; k < 3; ++k) ok = ok && !((need >> k & 1) && n_rows > 0 && !src[k]);
    if (!ok) return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    int rc = MGP_OK;
    {
        State st;
        DevBuf buf[3];
        const size_t npos = (size_t)n_rows * (size_t)mito_len;
        for (int k = 0; k < 3 && rc == MGP_OK; ++k)
            if (need >> k & 1) rc = buf[k].ensure(npos * row_bytes[k] + 64);
        for (int k = 0; k < 3 && rc == MGP_OK && npos; ++k)
            if ((need >> k & 1) &&
                hipMemcpy(buf[k].p, src[k], npos * row_bytes[k], hipMemcpyHostToDevice) != hipSuccess)
                rc = set_err(MGP_E_HIP, std::string(who) + ": upload failed");
        const txtgz::Rows rows{nullptr, nullptr, nullptr, buf[0].as<uint32_t>(), buf[2].as<uint32_t>(), mito_len,
                               mito_len, 1};
        const qc::Tn5 t{nullptr, buf[1].as<uint32_t>()};
        if (rc == MGP_OK) rc = job(st, s, rows, t);
        (void)hipStreamSynchronize(s);
    }
    (void)hipStreamDestroy(s);
    return rc;
}

// The clustering and graph calls, and mgp_h5_tiles_rows: job(state, stream) on `device` with a
// stream and a State of the call's own, freed once that stream is idle.
template <class State = ClusterState, class Job>
static int cl_call(int device, Job&& job) {
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    int rc;
    {
        State st;
        rc = job(st, s);
        (void)hipStreamSynchronize(s);
    }
    (void)hipStreamDestroy(s);
    return rc;
}

extern "C" {

// ---------------------------------------------------------------------------
// mgp_txt_gz: the txt count files formatted and deflated on the device
// (IncrementalTextWriter.write_cell + finalize's gzip -9, writers.py:430-486)
// ---------------------------------------------------------------------------
static int txt_run(TxtState& st, hipStream_t s, const txtgz::Rows& rows, int32_t n_rows, const mgp_txt_gz* job) {
    using namespace txtgz;
    const int64_t n = job->n_cells;
    if (n < 0 || (n > 0 && (!job->cells || !job->names || !job->name_off || !job->member_bytes)))
        return set_err(MGP_E_INVALID, "mgp_txt_gz: bad arguments");
    st.n = n;
    st.total = 0;
    if (n == 0) return MGP_OK;
    if (n > (int64_t)1 << 26) return set_err(MGP_E_INVALID, "mgp_txt_gz: too many cells for one call");
    for (int64_t k = 0; k < n; ++k) {
        if (job->cells[k] < 0 || job->cells[k] >= n_rows) return set_err(MGP_E_INVALID, "mgp_txt_gz: cell out of range");
        const int64_t bl = job->name_off[k + 1] - job->name_off[k];
        if (bl < 0 || bl > 4096 || job->name_off[k] < 0)
            return set_err(MGP_E_INVALID, "mgp_txt_gz: barcode names of 0..4096 bytes");
    }
    const int64_t nm = kFiles * n;
    const size_t nbytes = (size_t)job->name_off[n];
    MGP_TRY(st.cells.ensure((size_t)n * 4));
    MGP_TRY(st.names.ensure(nbytes + 1));
    MGP_TRY(st.name_off.ensure((size_t)(n + 1) * 8));
    MGP_TRY(st.sizes.ensure((size_t)nm * 8));
    MGP_TRY(st.nlines.ensure((size_t)nm * 8));
    MGP_TRY(st.offs.ensure((size_t)3 * (nm + 1) * 8));
    MGP_TRY(st.member_bytes.ensure((size_t)nm * 4));
    MGP_TRY(st.dst_off.ensure((size_t)nm * 8));
    if (!st.shift_ready) {
        std::vector<uint32_t> M(txtgz::kShiftPow * 32);
        crc_shift_matrices(M.data());
        MGP_TRY(st.crc_shift.ensure(M.size() * 4));
        HIP_TRY(hipMemcpy(st.crc_shift.p, M.data(), M.size() * 4, hipMemcpyHostToDevice));
        st.shift_ready = true;
    }
    HIP_TRY(hipMemcpyAsync(st.cells.p, job->cells, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (nbytes) HIP_TRY(hipMemcpyAsync(st.names.p, job->names, nbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(st.name_off.p, job->name_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
    Job jb{rows, n, st.cells.as<int32_t>(), st.names.as<char>(), st.name_off.as<int64_t>()};
    if (txt_sizes(jb, st.sizes.as<uint64_t>(), st.nlines.as<uint64_t>(), s) != 0)
        return set_err(MGP_E_HIP, "mgp_txt_gz: size kernel launch failed");
    std::vector<uint64_t> sz((size_t)nm), nl((size_t)nm), offs((size_t)3 * (nm + 1));
    HIP_TRY(hipMemcpyAsync(sz.data(), st.sizes.p, (size_t)nm * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nl.data(), st.nlines.p, (size_t)nm * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t* to = offs.data();
    uint64_t* lo = to + nm + 1;
    uint64_t* oo = lo + nm + 1;
    to[0] = lo[0] = oo[0] = 0;
    for (int64_t m = 0; m < nm; ++m) {
        to[m + 1] = to[m] + ((sz[(size_t)m] + 15) & ~uint64_t(15));  // (aligned: the parse loads 16 bytes)
        lo[m + 1] = lo[m] + nl[(size_t)m];
        oo[m + 1] = oo[m] + out_bound(sz[(size_t)m]);
        if (job->text_bytes) job->text_bytes[m] = (int64_t)sz[(size_t)m];
    }
    MGP_TRY(st.text.ensure(to[nm] + 256));  // (slack: a parse block reads up to 31 positions past a text)
    MGP_TRY(st.tok.ensure(4 * to[nm] + 1024));
    MGP_TRY(st.lines.ensure(12 * lo[nm] + 64));
    MGP_TRY(st.out.ensure(oo[nm] + 64));
    HIP_TRY(hipMemcpyAsync(st.offs.p, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, s));
    Scratch sc{};
    sc.text_off = st.offs.as<uint64_t>();
    sc.text_n = st.sizes.as<uint64_t>();
    sc.line_off = sc.text_off + nm + 1;
    sc.out_off = sc.line_off + nm + 1;
    sc.text = st.text.as<uint8_t>();
    sc.tok = st.tok.as<uint32_t>();
    sc.lines = st.lines.as<uint32_t>();
    sc.out = st.out.as<uint32_t>();
    sc.member_bytes = st.member_bytes.as<uint32_t>();
    sc.crc_shift = st.crc_shift.as<uint32_t>();
    MGP_TRY(st.seg.ensure((size_t)nm * 257 * 4));
    MGP_TRY(st.crc.ensure((size_t)nm * 4));
    sc.seg = st.seg.as<uint32_t>();
    sc.crc = st.crc.as<uint32_t>();
    sc.prof = nullptr;
    const bool prof = std::getenv("MGP_TXT_PROF") != nullptr;
    if (prof) {
        MGP_TRY(st.prof.ensure((size_t)nm * 64));
        HIP_TRY(hipMemsetAsync(st.prof.p, 0, (size_t)nm * 64, s));
        sc.prof = st.prof.as<uint64_t>();
    }
    if (txt_deflate(jb, sc, s) != 0) return set_err(MGP_E_HIP, "mgp_txt_gz: deflate kernel launch failed");
    if (prof) {  // per-phase means over the members that have text (us), to stderr
        std::vector<uint64_t> pr((size_t)nm * 8);
        HIP_TRY(hipMemcpyAsync(pr.data(), st.prof.p, pr.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // stamps: 0 format start, 1 format end, 2 match end, 3 parse end, 4 code end; each
        // kernel's span over all members (first start to last end) and the mean per member
        double mean[3] = {0, 0, 0};
        uint64_t lo[3] = {UINT64_MAX, UINT64_MAX, UINT64_MAX}, hi[3] = {0, 0, 0};
        int64_t cnt = 0;
        for (int64_t m = 0; m < nm; ++m) {
            const uint64_t* q = pr.data() + m * 8;
            if (!q[4]) continue;
            ++cnt;
            mean[0] += (double)(q[1] - q[0]) * 0.01;
            lo[0] = std::min(lo[0], q[0]);
            hi[0] = std::max(hi[0], q[1]);
            hi[1] = std::max(hi[1], q[2]);
            hi[2] = std::max(hi[2], q[4]);
            mean[2] += (double)(q[4] - q[3]) * 0.01;
        }
        // format phases per member: 0 start, 5 sizes + scan, 6 text written, 7 own CRC, 1 end
        double fp[4] = {0, 0, 0, 0};
        for (int64_t m = 0; m < nm; ++m) {
            const uint64_t* q = pr.data() + m * 8;
            if (!q[4]) continue;
            fp[0] += (double)(q[5] - q[0]) * 0.01;
            fp[1] += (double)(q[6] - q[5]) * 0.01;
            fp[2] += (double)(q[7] - q[6]) * 0.01;
            fp[3] += (double)(q[1] - q[7]) * 0.01;
        }
        std::fprintf(stderr, "[mgp_txt_gz] %lld members: format %.1f ms (%.1f us per member: sizes %.1f, text %.1f, "
                     "crc %.1f, combine %.1f), match %.1f ms, code %.1f ms (tail %.1f us per member)\n", (long long)cnt,
                     (hi[0] - lo[0]) * 1e-5, mean[0] / cnt, fp[0] / cnt, fp[1] / cnt, fp[2] / cnt, fp[3] / cnt,
                     (hi[1] - hi[0]) * 1e-5, (hi[2] - hi[1]) * 1e-5, mean[2] / cnt);
    }
    std::vector<uint32_t> mb((size_t)nm);
    HIP_TRY(hipMemcpyAsync(mb.data(), st.member_bytes.p, (size_t)nm * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint64_t> dst((size_t)nm);
    uint64_t tot = 0;
    for (int64_t m = 0; m < nm; ++m) {
        dst[(size_t)m] = tot;
        tot += mb[(size_t)m];
        job->member_bytes[m] = mb[(size_t)m];
    }
    MGP_TRY(st.packed.ensure(tot + 64));
    HIP_TRY(hipMemcpyAsync(st.dst_off.p, dst.data(), (size_t)nm * 8, hipMemcpyHostToDevice, s));
    if (txt_pack(sc, nm, st.dst_off.as<uint64_t>(), st.packed.as<uint8_t>(), s) != 0)
        return set_err(MGP_E_HIP, "mgp_txt_gz: pack kernel launch failed");
    HIP_TRY(hipStreamSynchronize(s));
    st.total = tot;
    return MGP_OK;
}

int mgp_txt_gz_run(mgp_ctx* ctx, mgp_txt_gz* job, int64_t* total_bytes) {
    if (!ctx || !job) return set_err(MGP_E_INVALID, "null ctx/job");
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_txt_gz: no run to write", &r));
    MGP_TRY(txt_run(r.jobs->txt, r.stream, r.rows, r.n_cells, job));
    if (total_bytes) *total_bytes = (int64_t)r.jobs->txt.total;
    return MGP_OK;
}

int mgp_txt_gz_fetch(mgp_ctx* ctx, uint8_t* dst, int64_t cap) {
    int device = 0;
    const RowJobs* jobs = ctx ? ctx_jobs(ctx, &device) : nullptr;
    if (!ctx || (!dst && jobs->txt.total)) return set_err(MGP_E_INVALID, "null ctx/dst");
    if (cap < (int64_t)jobs->txt.total) return set_err(MGP_E_INVALID, "mgp_txt_gz_fetch: destination too small");
    HIP_TRY(hipSetDevice(device));
    if (jobs->txt.total) HIP_TRY(hipMemcpy(dst, jobs->txt.packed.p, jobs->txt.total, hipMemcpyDeviceToHost));
    return MGP_OK;
}

// ---------------------------------------------------------------------------
// mgp_h5_tiles: the HDF5 count datasets' chunks deflated on the device
// (IncrementalHDF5Writer, writers.py:60-131: 11 u16 planes, gzip-4 chunks of 1000 x 100)
// ---------------------------------------------------------------------------
// the arguments of `job` over n_cells rows of L positions (before anything is allocated)
static int h5_check(const mgp_h5_tiles* job, int L, int32_t n_cells) {
    const int64_t nco = job->n_cols;
    const int crow = job->chunk_rows, ccol = job->chunk_cols;
    if (nco < 0 || crow <= 0 || ccol <= 0 || (int64_t)crow * ccol > (1 << 22) || !job->chunk_bytes ||
        (nco > 0 && !job->cell_of_col))
        return set_err(MGP_E_INVALID, "mgp_h5_tiles: bad arguments");
    const int64_t ncc_all = (nco + ccol - 1) / ccol;
    const int lo = job->col_chunk_lo, hi = job->col_chunk_hi;
    if (lo < 0 || hi < lo || hi > ncc_all) return set_err(MGP_E_INVALID, "mgp_h5_tiles: column chunks out of range");
    const int64_t nch = (int64_t)txtgz::kPlanes * ((L + crow - 1) / crow) * (hi - lo);
    if (nch > (int64_t)1 << 20) return set_err(MGP_E_INVALID, "mgp_h5_tiles: too many chunks for one call");
    if (nch == 0) return MGP_OK;
    for (int64_t j = 0; j < nco; ++j)
        if (job->cell_of_col[j] < -1 || job->cell_of_col[j] >= n_cells)
            return set_err(MGP_E_INVALID, "mgp_h5_tiles: cell of a column out of range");
    return MGP_OK;
}

// the streams of `job` from the 16-bit planes c16 / t16 / d16 ([n_cells][L]) into st.packed
// (st.total bytes; job->chunk_bytes and col_sums filled)
static int h5_run(H5State& st, hipStream_t s, const uint4* c16, const uint32_t* t16, const uint16_t* d16, int L,
                  int32_t n_cells, mgp_h5_tiles* job) {
    using namespace txtgz;
    st.total = 0;
    MGP_TRY(h5_check(job, L, n_cells));
    const int64_t nco = job->n_cols;
    const int crow = job->chunk_rows, ccol = job->chunk_cols;
    const int lo = job->col_chunk_lo, hi = job->col_chunk_hi;
    const int nrc = (L + crow - 1) / crow, ncc = hi - lo;
    const int64_t nch = (int64_t)kPlanes * nrc * ncc;
    if (nch == 0) return MGP_OK;
    const uint64_t chunk_raw = (uint64_t)crow * ccol * 2, stride = out_bound(chunk_raw);
    const uint64_t raw_stride = (chunk_raw + 15) & ~uint64_t(15);
    MGP_TRY(st.coc.ensure((size_t)std::max<int64_t>(nco, 1) * 4));
    MGP_TRY(st.raw.ensure((size_t)(nch * raw_stride) + 64));
    MGP_TRY(st.tok.ensure((size_t)(nch * h5_tok_words(chunk_raw)) * 4 + 64));
    MGP_TRY(st.out.ensure((size_t)(nch * stride) + 64));
    MGP_TRY(st.out_off.ensure((size_t)nch * 8));
    MGP_TRY(st.chunk_bytes.ensure((size_t)nch * 4));
    MGP_TRY(st.dst_off.ensure((size_t)nch * 8));
    MGP_TRY(st.sums.ensure((size_t)3 * L * 8));
    HIP_TRY(hipMemsetAsync(st.sums.p, 0, (size_t)3 * L * 8, s));
    std::vector<uint64_t> oo((size_t)nch);
    for (int64_t k = 0; k < nch; ++k) oo[(size_t)k] = (uint64_t)k * stride;
    if (nco) HIP_TRY(hipMemcpyAsync(st.coc.p, job->cell_of_col, (size_t)nco * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(st.out_off.p, oo.data(), (size_t)nch * 8, hipMemcpyHostToDevice, s));
    H5Job jb{c16, t16, d16, L, st.coc.as<int32_t>(), nco, crow, ccol, nrc, lo, ncc,
             st.sums.as<unsigned long long>()};
    H5Scratch sc{st.raw.as<uint8_t>(), st.tok.as<uint32_t>(), st.out.as<uint32_t>(), st.out_off.as<uint64_t>(),
                 st.chunk_bytes.as<uint32_t>(), chunk_raw, stride, raw_stride, h5_tok_words(chunk_raw), nullptr};
    const bool prof = std::getenv("MGP_H5_PROF") != nullptr;
    if (prof) {
        MGP_TRY(st.prof.ensure((size_t)nch * 64));
        HIP_TRY(hipMemsetAsync(st.prof.p, 0, (size_t)nch * 64, s));
        sc.prof = st.prof.as<uint64_t>();
    }
    if (h5_deflate(jb, sc, s) != 0) return set_err(MGP_E_HIP, "mgp_h5_tiles: deflate kernel launch failed");
    if (prof) {  // per-phase means over the chunks (us) and the code kernel's span, to stderr
        // stamps: 0 start, 1 parse, 2 adler, 3 end; 4 lit/dist lengths, 5 header, 6 sizes (deflate_block)
        std::vector<uint64_t> pr((size_t)nch * 8);
        HIP_TRY(hipMemcpyAsync(pr.data(), st.prof.p, pr.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const int ord[7] = {0, 1, 2, 4, 5, 6, 3};  // phases in time order
        double m[6] = {0, 0, 0, 0, 0, 0};
        uint64_t a = UINT64_MAX, b = 0;
        for (int64_t k = 0; k < nch; ++k) {
            const uint64_t* q = pr.data() + k * 8;
            for (int i = 0; i < 6; ++i) m[i] += (double)(q[ord[i + 1]] - q[ord[i]]) * 0.01;
            a = std::min(a, q[0]);
            b = std::max(b, q[3]);
        }
        std::fprintf(stderr, "[mgp_h5_tiles] %lld chunks: parse %.1f us, adler %.1f, huffman %.1f, header %.1f, "
                     "sizes %.1f, encode %.1f us per chunk; span %.2f ms\n", (long long)nch, m[0] / nch, m[1] / nch,
                     m[2] / nch, m[3] / nch, m[4] / nch, m[5] / nch, (b - a) * 1e-5);
    }
    std::vector<uint32_t> cb((size_t)nch);
    HIP_TRY(hipMemcpyAsync(cb.data(), st.chunk_bytes.p, (size_t)nch * 4, hipMemcpyDeviceToHost, s));
    if (job->col_sums)
        HIP_TRY(hipMemcpyAsync(job->col_sums, st.sums.p, (size_t)3 * L * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint64_t> dst((size_t)nch);
    uint64_t tot = 0;
    for (int64_t k = 0; k < nch; ++k) {
        dst[(size_t)k] = tot;
        tot += cb[(size_t)k];
        job->chunk_bytes[k] = cb[(size_t)k];
    }
    MGP_TRY(st.packed.ensure(tot + 64));
    HIP_TRY(hipMemcpyAsync(st.dst_off.p, dst.data(), (size_t)nch * 8, hipMemcpyHostToDevice, s));
    if (h5_pack(sc, nch, st.dst_off.as<uint64_t>(), st.packed.as<uint8_t>(), s) != 0)
        return set_err(MGP_E_HIP, "mgp_h5_tiles: pack kernel launch failed");
    HIP_TRY(hipStreamSynchronize(s));
    st.total = tot;
    return MGP_OK;
}

int mgp_h5_tiles_run(mgp_ctx* ctx, mgp_h5_tiles* job, int64_t* total_bytes) {
    if (!ctx || !job) return set_err(MGP_E_INVALID, "null ctx/job");
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_h5_tiles: no run to write", &r));
    MGP_TRY(h5_run(r.jobs->h5, r.stream, r.rows.c16, r.tn5.t16, r.rows.d16, r.rows.L, r.n_cells, job));
    if (total_bytes) *total_bytes = (int64_t)r.jobs->h5.total;
    return MGP_OK;
}

int mgp_h5_tiles_fetch(mgp_ctx* ctx, uint8_t* dst, int64_t cap) {
    int device = 0;
    const RowJobs* jobs = ctx ? ctx_jobs(ctx, &device) : nullptr;
    if (!ctx || (!dst && jobs->h5.total)) return set_err(MGP_E_INVALID, "null ctx/dst");
    if (cap < (int64_t)jobs->h5.total) return set_err(MGP_E_INVALID, "mgp_h5_tiles_fetch: destination too small");
    HIP_TRY(hipSetDevice(device));
    if (jobs->h5.total) HIP_TRY(hipMemcpy(dst, jobs->h5.packed.p, jobs->h5.total, hipMemcpyDeviceToHost));
    return MGP_OK;
}

// The caller's u32 rows saturated and packed on the host into the run's 16-bit layout (one
// uint4 of (fwd | rev << 16) pairs, one tn5 word and one u16 depth per position), uploaded,
// and h5_run on them under a stream and a state of the call's own (cl_call).
int mgp_h5_tiles_rows(int device, const uint32_t* counts, const uint32_t* tn5, const uint32_t* depth, int32_t n_rows,
                      int32_t mito_len, mgp_h5_tiles* job, uint8_t* dst, int64_t cap, int64_t* total_bytes) {
    const std::string who = "mgp_h5_tiles_rows";
    if (!job || n_rows < 0 || mito_len <= 0 || (n_rows > 0 && (!counts || !tn5 || !depth)))
        return set_err(MGP_E_INVALID, who + ": bad arguments");
    return cl_call<H5State>(device, [&](H5State& st, hipStream_t s) {
        MGP_TRY(h5_check(job, mito_len, n_rows));
        const size_t npos = (size_t)n_rows * (size_t)mito_len;
        std::vector<uint32_t> c16(npos * 4), t16(npos);
        std::vector<uint16_t> d16(npos);
        auto sat = [](uint32_t v) -> uint32_t { return v < 65535u ? v : 65535u; };
        for (size_t P = 0; P < npos; ++P) {
            for (int q = 0; q < 4; ++q)
                c16[4 * P + q] = sat(counts[8 * P + 2 * q]) | sat(counts[8 * P + 2 * q + 1]) << 16;
            t16[P] = sat(tn5[2 * P]) | sat(tn5[2 * P + 1]) << 16;
            d16[P] = (uint16_t)sat(depth[P]);
        }
        DevBuf bc, bt, bd;
        MGP_TRY(bc.ensure(npos * 16 + 64));
        MGP_TRY(bt.ensure(npos * 4 + 64));
        MGP_TRY(bd.ensure(npos * 2 + 64));
        if (npos && (hipMemcpy(bc.p, c16.data(), npos * 16, hipMemcpyHostToDevice) != hipSuccess ||
                     hipMemcpy(bt.p, t16.data(), npos * 4, hipMemcpyHostToDevice) != hipSuccess ||
                     hipMemcpy(bd.p, d16.data(), npos * 2, hipMemcpyHostToDevice) != hipSuccess))
            return set_err(MGP_E_HIP, who + ": upload failed");
        const int rc = h5_run(st, s, bc.as<uint4>(), bt.as<uint32_t>(), bd.as<uint16_t>(), mito_len, n_rows, job);
        (void)hipStreamSynchronize(s);  // (before the rows' buffers go)
        if (rc != MGP_OK) return rc;
        if (total_bytes) *total_bytes = (int64_t)st.total;
        if ((int64_t)st.total > cap) return set_err(MGP_E_INVALID, who + ": destination too small");
        if (st.total && !dst) return set_err(MGP_E_INVALID, who + ": bad arguments");
        if (st.total && hipMemcpy(dst, st.packed.p, st.total, hipMemcpyDeviceToHost) != hipSuccess)
            return set_err(MGP_E_HIP, who + ": download failed");
        return (int)MGP_OK;
    });
}

int mgp_txt_gz_rows(int device, const uint32_t* counts, const uint32_t* depth, int32_t n_rows, int32_t mito_len,
                    mgp_txt_gz* job, uint8_t* dst, int64_t cap, int64_t* total_bytes) {
    const char* who = "mgp_txt_gz_rows";
    if (!job) return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    const HostRows h{counts, nullptr, depth, n_rows, mito_len};
    return on_rows<TxtState>(device, who, PL_COUNTS | PL_DEPTH, h,
                             [&](TxtState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5&) {
        MGP_TRY(txt_run(st, s, rows, n_rows, job));
        if (total_bytes) *total_bytes = (int64_t)st.total;
        if ((int64_t)st.total > cap) return set_err(MGP_E_INVALID, std::string(who) + ": destination too small");
        if (st.total && hipMemcpy(dst, st.packed.p, st.total, hipMemcpyDeviceToHost) != hipSuccess)
            return set_err(MGP_E_HIP, std::string(who) + ": download failed");
        return (int)MGP_OK;
    });
}

// ---------------------------------------------------------------------------
// mgp_variant_* / mgp_allele_freq_*: variant statistics and heteroplasmy from the count
// rows (identify_variants / calculate_allele_freq, R/mgatk2_functions.R:282-372)
// ---------------------------------------------------------------------------
// MGP_VAR_PROF: the kernels' device time between two events of the call's stream, to stderr
struct VarProf {
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    explicit VarProf(hipStream_t st) : s(st) {
        if (!std::getenv("MGP_VAR_PROF")) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
        (void)hipEventRecord(a, s);
    }
    void stop() {
        if (a && b) (void)hipEventRecord(b, s);
    }
    // (after the stream is synchronised)
    void report(const char* who, const char* what, int64_t n, int64_t m) {
        float ms = 0;
        if (a && b && hipEventElapsedTime(&ms, a, b) == hipSuccess)
            std::fprintf(stderr, "[%s] %lld x %lld %s: kernels %.3f ms\n", who, (long long)n, (long long)m, what, ms);
    }
    // (after the stream is synchronised) the milliseconds alone, 0 when not measured
    float ms() {
        float v = 0;
        return a && b && hipEventElapsedTime(&v, a, b) == hipSuccess ? v : 0.0f;
    }
    ~VarProf() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

// the job's population on the device: *cells = its list (null: rows 0..n-1), *n its size
static int var_population(DevBuf& buf, hipStream_t s, int32_t n_rows, const mgp_variant_job* job, const char* who,
                          const int32_t** cells, int64_t* n) {
    if (!job || job->low_coverage_threshold < 0 || (job->cells && job->n_cells < 0))
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    *n = job->cells ? job->n_cells : (int64_t)n_rows;
    *cells = nullptr;
    if (*n > variants::kMaxCells)
        return set_err(MGP_E_INVALID, std::string(who) + ": more than 65536 cells in one call (the exactness bound of "
                                                         "the u64 moments); split the population and add the moments");
    if (!job->cells) return MGP_OK;
    for (int64_t k = 0; k < *n; ++k)
        if (job->cells[k] < -1 || job->cells[k] >= n_rows)
            return set_err(MGP_E_INVALID, std::string(who) + ": cell out of range");
    MGP_TRY(buf.ensure((size_t)std::max<int64_t>(*n, 1) * 4));
    if (*n) HIP_TRY(hipMemcpyAsync(buf.p, job->cells, (size_t)*n * 4, hipMemcpyHostToDevice, s));
    *cells = buf.as<int32_t>();
    return MGP_OK;
}

static int var_moments(VarState& st, hipStream_t s, const txtgz::Rows& rows, int32_t n_rows, const mgp_variant_job* job,
                       mgp_variant_moments* out) {
    using namespace variants;
    const char* who = "mgp_variant_moments";
    if (!out || !out->n_det || !out->n_conf || !out->s_total || !out->s_cov || !out->m || !out->sf || !out->sr ||
        !out->sff || !out->srr || !out->sfr || !out->n_low || !out->s_af)
        return set_err(MGP_E_INVALID, std::string(who) + ": null output array");
    const int32_t* cells = nullptr;
    int64_t n = 0;
    MGP_TRY(var_population(st.cells, s, n_rows, job, who, &cells, &n));
    const size_t L = (size_t)rows.L, plane = L * 4;
    MGP_TRY(st.acc.ensure(acc_words(rows.L) * 8));
    MGP_TRY(st.part.ensure((size_t)slabs(n) * plane * 8));
    MGP_TRY(st.f64.ensure(plane * 8));
    MGP_TRY(st.bad.ensure(4));
    VarProf prof(s);
    if (moments(rows, cells, n, (uint32_t)job->low_coverage_threshold, st.acc.as<unsigned long long>(),
                st.part.as<double>(), st.f64.as<double>(), st.bad.as<uint32_t>(), s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    prof.stop();
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, st.bad.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    prof.report(who, "cells x positions", n, rows.L);
    if (bad)
        return set_err(MGP_E_INVALID, std::string(who) + ": a fwd or rev count of the population is 2^24 or more "
                                                         "(the exactness bound of the u64 moments)");
    uint64_t* dst[F_N] = {out->n_det, out->n_conf, out->s_total, out->m, out->sf, out->sr, out->sff, out->srr, out->sfr};
    const uint64_t* acc = st.acc.as<uint64_t>();
    for (int k = 0; k < F_N; ++k) HIP_TRY(hipMemcpyAsync(dst[k], acc + k * plane, plane * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out->s_cov, acc + acc_scov(rows.L), L * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out->n_low, acc + acc_nlow(rows.L), L * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out->s_af, st.f64.p, plane * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MGP_OK;
}

static int var_dev2(VarState& st, hipStream_t s, const txtgz::Rows& rows, int32_t n_rows, const mgp_variant_job* job,
                    const double* mean_af, double* out_dev2) {
    using namespace variants;
    const char* who = "mgp_variant_dev2";
    if (!mean_af || !out_dev2) return set_err(MGP_E_INVALID, std::string(who) + ": null mean_af / out_dev2");
    const int32_t* cells = nullptr;
    int64_t n = 0;
    MGP_TRY(var_population(st.cells, s, n_rows, job, who, &cells, &n));
    const size_t plane = (size_t)rows.L * 4;
    MGP_TRY(st.part.ensure((size_t)slabs(n) * plane * 8));
    MGP_TRY(st.f64.ensure(plane * 8));
    MGP_TRY(st.mu.ensure(plane * 8));
    HIP_TRY(hipMemcpyAsync(st.mu.p, mean_af, plane * 8, hipMemcpyHostToDevice, s));
    VarProf prof(s);
    if (dev2(rows, cells, n, (uint32_t)job->low_coverage_threshold, st.mu.as<double>(), st.part.as<double>(),
             st.f64.as<double>(), s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    prof.stop();
    HIP_TRY(hipMemcpyAsync(out_dev2, st.f64.p, plane * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    prof.report(who, "cells x positions", n, rows.L);
    return MGP_OK;
}

static int var_allele_freq(VarState& st, hipStream_t s, const txtgz::Rows& rows, int32_t n_rows,
                           const mgp_variant_job* job, int64_t n_var, const int32_t* pos, const int32_t* base,
                           int32_t min_coverage, double* out) {
    const char* who = "mgp_allele_freq";
    if (n_var < 0 || min_coverage < 0 || (n_var > 0 && (!pos || !base)))
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    const int32_t* cells = nullptr;
    int64_t n = 0;
    MGP_TRY(var_population(st.cells, s, n_rows, job, who, &cells, &n));
    for (int64_t v = 0; v < n_var; ++v)
        if (pos[v] < 0 || pos[v] >= rows.L || base[v] < 0 || base[v] > 3)
            return set_err(MGP_E_INVALID, std::string(who) + ": variant position or base out of range");
    if (n == 0 || n_var == 0) return MGP_OK;
    if (!out) return set_err(MGP_E_INVALID, std::string(who) + ": null output");
    if (n_var > ((int64_t)1 << 29) / n)
        return set_err(MGP_E_INVALID, std::string(who) + ": more than 2^29 values in one call; split the variants");
    const size_t vals = (size_t)n_var * (size_t)n;
    MGP_TRY(st.pos.ensure((size_t)n_var * 4));
    MGP_TRY(st.base.ensure((size_t)n_var * 4));
    MGP_TRY(st.out.ensure(vals * 8));
    HIP_TRY(hipMemcpyAsync(st.pos.p, pos, (size_t)n_var * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(st.base.p, base, (size_t)n_var * 4, hipMemcpyHostToDevice, s));
    VarProf prof(s);
    if (variants::gather(rows, cells, n, st.pos.as<int32_t>(), st.base.as<int32_t>(), n_var, (uint32_t)min_coverage,
                         st.out.as<double>(), s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    prof.stop();
    HIP_TRY(hipMemcpyAsync(out, st.out.p, vals * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    prof.report(who, "variants x cells", n_var, n);
    return MGP_OK;
}

int mgp_variant_moments_run(mgp_ctx* ctx, const mgp_variant_job* job, mgp_variant_moments* out) {
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_variant_moments_run: no run to read", &r));
    return var_moments(r.jobs->var, r.stream, r.rows, r.n_cells, job, out);
}

int mgp_variant_dev2_run(mgp_ctx* ctx, const mgp_variant_job* job, const double* mean_af, double* out_dev2) {
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_variant_dev2_run: no run to read", &r));
    return var_dev2(r.jobs->var, r.stream, r.rows, r.n_cells, job, mean_af, out_dev2);
}

int mgp_allele_freq_run(mgp_ctx* ctx, const mgp_variant_job* job, int64_t n_var, const int32_t* pos,
                        const int32_t* base, int32_t min_coverage, double* out) {
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_allele_freq_run: no run to read", &r));
    return var_allele_freq(r.jobs->var, r.stream, r.rows, r.n_cells, job, n_var, pos, base, min_coverage, out);
}

int mgp_variant_moments_rows(int device, const uint32_t* counts, const uint32_t* depth, int32_t n_rows, int32_t mito_len,
                             const mgp_variant_job* job, mgp_variant_moments* out) {
    const HostRows h{counts, nullptr, depth, n_rows, mito_len};
    return on_rows<VarState>(device, "mgp_variant_moments_rows", PL_COUNTS | PL_DEPTH, h,
                             [&](VarState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5&) {
        return var_moments(st, s, rows, n_rows, job, out);
    });
}

int mgp_variant_dev2_rows(int device, const uint32_t* counts, const uint32_t* depth, int32_t n_rows, int32_t mito_len,
                          const mgp_variant_job* job, const double* mean_af, double* out_dev2) {
    const HostRows h{counts, nullptr, depth, n_rows, mito_len};
    return on_rows<VarState>(device, "mgp_variant_dev2_rows", PL_COUNTS | PL_DEPTH, h,
                             [&](VarState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5&) {
        return var_dev2(st, s, rows, n_rows, job, mean_af, out_dev2);
    });
}

int mgp_allele_freq_rows(int device, const uint32_t* counts, const uint32_t* depth, int32_t n_rows, int32_t mito_len,
                         const mgp_variant_job* job, int64_t n_var, const int32_t* pos, const int32_t* base,
                         int32_t min_coverage, double* out) {
    const HostRows h{counts, nullptr, depth, n_rows, mito_len};
    return on_rows<VarState>(device, "mgp_allele_freq_rows", PL_COUNTS | PL_DEPTH, h,
                             [&](VarState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5&) {
        return var_allele_freq(st, s, rows, n_rows, job, n_var, pos, base, min_coverage, out);
    });
}

// ---------------------------------------------------------------------------
// mgp_group_moments_run / mgp_rows_group_moments: pseudobulk counts per cell group
// ---------------------------------------------------------------------------
// the pointers, checked before any device call
static int grp_pointers(const char* who, const mgp_variant_job* job, const int32_t* group,
                        const mgp_group_moments* out) {
    if (!job || !group || !out || !out->fwd || !out->rev || !out->cov || !out->n_det || !out->n_conf ||
        (job->cells && job->n_cells < 0))
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    return MGP_OK;
}

// everything a call is refused for before it allocates or launches
static int grp_check(const char* who, int32_t n_rows, const mgp_variant_job* job, const int32_t* group,
                     int32_t n_groups, int32_t max_item_cells, const mgp_group_moments* out) {
    MGP_TRY(grp_pointers(who, job, group, out));
    if (n_groups < 1 || n_groups > groups::kMaxGroups)
        return set_err(MGP_E_INVALID, std::string(who) + ": n_groups must be 1.." + std::to_string(groups::kMaxGroups) +
                                          " in one call; split the groups");
    if (max_item_cells < 0) return set_err(MGP_E_INVALID, std::string(who) + ": max_item_cells is negative");
    const int64_t n = job->cells ? job->n_cells : (int64_t)n_rows;
    if (n > variants::kMaxCells)
        return set_err(MGP_E_INVALID, std::string(who) + ": more than 65536 cells in one call (the exactness bound of "
                                                         "the u64 sums); split the population and add the results");
    for (int64_t k = 0; k < n; ++k) {
        if (group[k] < -1 || group[k] >= n_groups)
            return set_err(MGP_E_INVALID, std::string(who) + ": group label out of range");
        if (job->cells && (job->cells[k] < -1 || job->cells[k] >= n_rows))
            return set_err(MGP_E_INVALID, std::string(who) + ": cell out of range");
    }
    return MGP_OK;
}

// (after grp_check)
static int grp_moments(GroupState& st, hipStream_t s, const txtgz::Rows& rows, int32_t n_rows, const char* who,
                       const mgp_variant_job* job, const int32_t* group, int32_t n_groups, int32_t max_item_cells,
                       mgp_group_moments* out) {
    using namespace groups;
    const int64_t n = job->cells ? job->n_cells : (int64_t)n_rows;
    // the population sorted by group (a counting sort: stable), the unlabelled entries left out
    std::vector<int64_t> start((size_t)n_groups + 1, 0);
    for (int64_t k = 0; k < n; ++k)
        if (group[k] >= 0) ++start[(size_t)group[k] + 1];
    for (int32_t g = 0; g < n_groups; ++g) start[(size_t)g + 1] += start[(size_t)g];
    const int64_t n_lab = start[(size_t)n_groups];
    std::vector<int32_t> sorted((size_t)n_lab);
    {
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t k = 0; k < n; ++k)
            if (group[k] >= 0) sorted[(size_t)at[(size_t)group[k]]++] = job->cells ? job->cells[k] : (int32_t)k;
    }
    const int64_t cap = max_item_cells > 0 ? max_item_cells : item_cells(n_lab, rows.L);
    std::vector<Item> items;
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t a = start[(size_t)g], b = start[(size_t)g + 1];
        for (int64_t k = a; k < b; k += cap)
            items.push_back(Item{(int32_t)k, (int32_t)std::min(b, k + cap), g, b - a <= cap ? 1 : 0});
    }
    const size_t L = (size_t)rows.L, gl = (size_t)n_groups * L;
    int rc = st.acc.ensure(acc_bytes(n_groups, rows.L));
    if (rc == MGP_OK) rc = st.cells.ensure((size_t)std::max<int64_t>(n_lab, 1) * 4);
    if (rc == MGP_OK) rc = st.items.ensure(std::max<size_t>(items.size(), 1) * sizeof(Item));
    if (rc == MGP_OK) rc = st.bad.ensure(4);
    if (rc != MGP_OK) {
        st.release();
        return rc;
    }
    const Acc acc = acc_of(st.acc.p, n_groups, rows.L);
    HIP_TRY(hipMemsetAsync(st.acc.p, 0, acc_bytes(n_groups, rows.L), s));
    HIP_TRY(hipMemsetAsync(st.bad.p, 0, 4, s));
    VarProf prof(s);
    if (!items.empty()) {
        HIP_TRY(hipMemcpyAsync(st.cells.p, sorted.data(), (size_t)n_lab * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(st.items.p, items.data(), items.size() * sizeof(Item), hipMemcpyHostToDevice, s));
        if (moments(rows, st.cells.as<int32_t>(), st.items.as<Item>(), (int64_t)items.size(), acc, st.bad.as<uint32_t>(),
                    s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    }
    prof.stop();
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, st.bad.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    prof.report(who, "cells x groups", n_lab, n_groups);
    if (bad)
        return set_err(MGP_E_INVALID, std::string(who) + ": a fwd or rev count of the population is 2^24 or more "
                                                         "(the exactness bound of the u64 sums)");
    HIP_TRY(hipMemcpyAsync(out->fwd, acc.fwd, gl * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out->rev, acc.rev, gl * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out->cov, acc.cov, gl * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out->n_det, acc.n_det, gl * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out->n_conf, acc.n_conf, gl * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MGP_OK;
}

int mgp_group_moments_run(mgp_ctx* ctx, const mgp_variant_job* job, const int32_t* group, int32_t n_groups,
                          int32_t max_item_cells, mgp_group_moments* out) {
    const char* who = "mgp_group_moments_run";
    if (!ctx) return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    MGP_TRY(grp_pointers(who, job, group, out));
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_group_moments_run: no run to read", &r));
    MGP_TRY(grp_check(who, r.n_cells, job, group, n_groups, max_item_cells, out));
    return grp_moments(r.jobs->grp, r.stream, r.rows, r.n_cells, who, job, group, n_groups, max_item_cells, out);
}

int mgp_rows_group_moments(int device, const uint32_t* counts, const uint32_t* depth, int32_t n_rows, int32_t mito_len,
                           const mgp_variant_job* job, const int32_t* group, int32_t n_groups, int32_t max_item_cells,
                           mgp_group_moments* out) {
    const char* who = "mgp_rows_group_moments";
    MGP_TRY(grp_check(who, n_rows, job, group, n_groups, max_item_cells, out));
    const HostRows h{counts, nullptr, depth, n_rows, mito_len};
    return on_rows<GroupState>(device, who, PL_COUNTS | PL_DEPTH, h,
                               [&](GroupState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5&) {
        return grp_moments(st, s, rows, n_rows, who, job, group, n_groups, max_item_cells, out);
    });
}

// ---------------------------------------------------------------------------
// mgp_cell_coverage_* / mgp_position_*: coverage QC from the count rows
// (calculate_cell_coverage_stats ... calculate_transposition_stats, R/mgatk2_functions.R:138-280)
// ---------------------------------------------------------------------------
static int qc_sum_bounds(const txtgz::Rows& rows, const char* who) {
    if (rows.L > qc::kMaxL)
        return set_err(MGP_E_INVALID, std::string(who) + ": more than 65536 positions (the exactness bound of the u64 sums)");
    return MGP_OK;
}

static int qc_bad(QcState& st, hipStream_t s, const char* who) {
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, st.bad.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad)
        return set_err(MGP_E_INVALID, std::string(who) + ": a depth or count of the population is 2^24 or more (the "
                                                         "exactness bound of the u64 sums)");
    return MGP_OK;
}

static int qc_cell_coverage(QcState& st, hipStream_t s, const txtgz::Rows& rows, int32_t n_rows,
                            const mgp_variant_job* job, mgp_cell_coverage* out) {
    using namespace qc;
    const char* who = "mgp_cell_coverage";
    if (!out) return set_err(MGP_E_INVALID, std::string(who) + ": null output");
    const int32_t* cells = nullptr;
    int64_t n = 0;
    MGP_TRY(var_population(st.cells, s, n_rows, job, who, &cells, &n));
    MGP_TRY(qc_sum_bounds(rows, who));
    if (n == 0) return MGP_OK;
    if (!out->s_depth || !out->s_depth2 || !out->max_depth || !out->n_covered || !out->n_10x || !out->n_50x ||
        !out->mid_lo || !out->mid_hi)
        return set_err(MGP_E_INVALID, std::string(who) + ": null output array");
    MGP_TRY(st.out64.ensure((size_t)n * CELL64_N * 8));
    MGP_TRY(st.out32.ensure((size_t)n * CELL32_N * 4));
    MGP_TRY(st.bad.ensure(4));
    VarProf prof(s);
    if (cell_stats(rows, cells, n, st.out64.as<unsigned long long>(), st.out32.as<uint32_t>(), st.bad.as<uint32_t>(),
                   s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    prof.stop();
    MGP_TRY(qc_bad(st, s, who));
    prof.report(who, "cells x positions", n, rows.L);
    std::vector<uint64_t> h64((size_t)n * CELL64_N);
    std::vector<uint32_t> h32((size_t)n * CELL32_N);
    HIP_TRY(hipMemcpyAsync(h64.data(), st.out64.p, h64.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h32.data(), st.out32.p, h32.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t* dst32[CELL32_N] = {out->max_depth, out->n_covered, out->n_10x, out->n_50x, out->mid_lo, out->mid_hi};
    for (int64_t k = 0; k < n; ++k) {
        out->s_depth[k] = h64[k * CELL64_N + CELL64_SD];
        out->s_depth2[k] = h64[k * CELL64_N + CELL64_SD2];
        for (int f = 0; f < CELL32_N; ++f) dst32[f][k] = h32[k * CELL32_N + f];
    }
    return MGP_OK;
}

static int qc_position_coverage(QcState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5& tn5,
                                int32_t n_rows, const mgp_variant_job* job, mgp_position_coverage* out) {
    using namespace qc;
    const char* who = "mgp_position_coverage";
    if (!out || !out->s_depth || !out->s_depth2 || !out->s_fwd || !out->s_rev || !out->s_tn5_fwd || !out->s_tn5_rev ||
        !out->tally || !out->n_covered || !out->n_10x || !out->n_50x || !out->n_tn5 || !out->max_depth)
        return set_err(MGP_E_INVALID, std::string(who) + ": null output array");
    const int32_t* cells = nullptr;
    int64_t n = 0;
    MGP_TRY(var_population(st.cells, s, n_rows, job, who, &cells, &n));
    MGP_TRY(qc_sum_bounds(rows, who));
    const size_t L = (size_t)rows.L;
    MGP_TRY(st.out64.ensure(L * POS64_N * 8));
    MGP_TRY(st.out32.ensure(L * POS32_N * 4));
    MGP_TRY(st.bad.ensure(4));
    VarProf prof(s);
    if (pos_stats(rows, tn5, cells, n, st.out64.as<unsigned long long>(), st.out32.as<uint32_t>(),
                  st.bad.as<uint32_t>(), s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    prof.stop();
    MGP_TRY(qc_bad(st, s, who));
    prof.report(who, "cells x positions", n, rows.L);
    uint64_t* dst64[POS64_TALLY] = {out->s_depth, out->s_depth2, out->s_fwd, out->s_rev, out->s_tn5_fwd, out->s_tn5_rev};
    uint32_t* dst32[POS32_N] = {out->n_covered, out->n_10x, out->n_50x, out->n_tn5, out->max_depth};
    const uint64_t* a64 = st.out64.as<uint64_t>();
    const uint32_t* a32 = st.out32.as<uint32_t>();
    for (int f = 0; f < POS64_TALLY; ++f) HIP_TRY(hipMemcpyAsync(dst64[f], a64 + f * L, L * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out->tally, a64 + POS64_TALLY * L, L * 4 * 8, hipMemcpyDeviceToHost, s));
    for (int f = 0; f < POS32_N; ++f) HIP_TRY(hipMemcpyAsync(dst32[f], a32 + f * L, L * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MGP_OK;
}

static int qc_depth_hist(QcState& st, hipStream_t s, const txtgz::Rows& rows, int32_t n_rows, const mgp_variant_job* job,
                         int32_t shift, const uint32_t* prefix, uint32_t* hist) {
    const char* who = "mgp_position_depth_hist";
    if (!hist || (shift != 0 && shift != 8 && shift != 16 && shift != 24) || (shift != 24 && !prefix))
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments (shift is 0, 8, 16 or 24)");
    const int32_t* cells = nullptr;
    int64_t n = 0;
    MGP_TRY(var_population(st.cells, s, n_rows, job, who, &cells, &n));
    const size_t L = (size_t)rows.L;
    MGP_TRY(st.in32.ensure(L * 4));
    MGP_TRY(st.hist.ensure(L * 256 * 4));
    if (shift != 24) HIP_TRY(hipMemcpyAsync(st.in32.p, prefix, L * 4, hipMemcpyHostToDevice, s));
    VarProf prof(s);
    if (qc::pos_depth_hist(rows, cells, n, shift, st.in32.as<uint32_t>(), st.hist.as<uint32_t>(), s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    prof.stop();
    HIP_TRY(hipMemcpyAsync(hist, st.hist.p, L * 256 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    prof.report(who, "cells x positions", n, rows.L);
    return MGP_OK;
}

static int qc_depth_next(QcState& st, hipStream_t s, const txtgz::Rows& rows, int32_t n_rows, const mgp_variant_job* job,
                         const uint32_t* v, uint32_t* n_le, uint32_t* next) {
    const char* who = "mgp_position_depth_next";
    if (!v || !n_le || !next) return set_err(MGP_E_INVALID, std::string(who) + ": null array");
    const int32_t* cells = nullptr;
    int64_t n = 0;
    MGP_TRY(var_population(st.cells, s, n_rows, job, who, &cells, &n));
    const size_t L = (size_t)rows.L;
    MGP_TRY(st.in32.ensure(L * 4));
    MGP_TRY(st.out32.ensure(L * 2 * 4));
    HIP_TRY(hipMemcpyAsync(st.in32.p, v, L * 4, hipMemcpyHostToDevice, s));
    uint32_t* o = st.out32.as<uint32_t>();
    VarProf prof(s);
    if (qc::pos_depth_next(rows, cells, n, st.in32.as<uint32_t>(), o, o + L, s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    prof.stop();
    HIP_TRY(hipMemcpyAsync(n_le, o, L * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(next, o + L, L * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    prof.report(who, "cells x positions", n, rows.L);
    return MGP_OK;
}

int mgp_cell_coverage_run(mgp_ctx* ctx, const mgp_variant_job* job, mgp_cell_coverage* out) {
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_cell_coverage_run: no run to read", &r));
    return qc_cell_coverage(r.jobs->qc, r.stream, r.rows, r.n_cells, job, out);
}

int mgp_position_coverage_run(mgp_ctx* ctx, const mgp_variant_job* job, mgp_position_coverage* out) {
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_position_coverage_run: no run to read", &r));
    return qc_position_coverage(r.jobs->qc, r.stream, r.rows, r.tn5, r.n_cells, job, out);
}

int mgp_position_depth_hist_run(mgp_ctx* ctx, const mgp_variant_job* job, int32_t shift, const uint32_t* prefix,
                                uint32_t* hist) {
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_position_depth_hist_run: no run to read", &r));
    return qc_depth_hist(r.jobs->qc, r.stream, r.rows, r.n_cells, job, shift, prefix, hist);
}

int mgp_position_depth_next_run(mgp_ctx* ctx, const mgp_variant_job* job, const uint32_t* v, uint32_t* n_le,
                                uint32_t* next) {
    RunRows r;
    MGP_TRY(run_rows(ctx, "mgp_position_depth_next_run: no run to read", &r));
    return qc_depth_next(r.jobs->qc, r.stream, r.rows, r.n_cells, job, v, n_le, next);
}

int mgp_cell_coverage_rows(int device, const uint32_t* depth, int32_t n_rows, int32_t mito_len,
                           const mgp_variant_job* job, mgp_cell_coverage* out) {
    const HostRows h{nullptr, nullptr, depth, n_rows, mito_len};
    return on_rows<QcState>(device, "mgp_cell_coverage_rows", PL_DEPTH, h,
                            [&](QcState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5&) {
        return qc_cell_coverage(st, s, rows, n_rows, job, out);
    });
}

int mgp_position_coverage_rows(int device, const uint32_t* counts, const uint32_t* tn5, const uint32_t* depth,
                               int32_t n_rows, int32_t mito_len, const mgp_variant_job* job,
                               mgp_position_coverage* out) {
    const HostRows h{counts, tn5, depth, n_rows, mito_len};
    return on_rows<QcState>(device, "mgp_position_coverage_rows", PL_COUNTS | PL_TN5 | PL_DEPTH, h,
                            [&](QcState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5& t) {
        return qc_position_coverage(st, s, rows, t, n_rows, job, out);
    });
}

int mgp_position_depth_hist_rows(int device, const uint32_t* depth, int32_t n_rows, int32_t mito_len,
                                 const mgp_variant_job* job, int32_t shift, const uint32_t* prefix, uint32_t* hist) {
    const HostRows h{nullptr, nullptr, depth, n_rows, mito_len};
    return on_rows<QcState>(device, "mgp_position_depth_hist_rows", PL_DEPTH, h,
                            [&](QcState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5&) {
        return qc_depth_hist(st, s, rows, n_rows, job, shift, prefix, hist);
    });
}

int mgp_position_depth_next_rows(int device, const uint32_t* depth, int32_t n_rows, int32_t mito_len,
                                 const mgp_variant_job* job, const uint32_t* v, uint32_t* n_le, uint32_t* next) {
    const HostRows h{nullptr, nullptr, depth, n_rows, mito_len};
    return on_rows<QcState>(device, "mgp_position_depth_next_rows", PL_DEPTH, h,
                            [&](QcState& st, hipStream_t s, const txtgz::Rows& rows, const qc::Tn5&) {
        return qc_depth_next(st, s, rows, n_rows, job, v, n_le, next);
    });
}

// ---------------------------------------------------------------------------
// mgp_pair_dist / mgp_hclust_dist / mgp_hclust: Euclidean pair distances and complete
// linkage of the heteroplasmy matrix's columns (pheatmap's dist() + hclust(), the step
// after calculate_allele_freq in R/mgatk2_qc_plots.R:121-139). No engine context: a call
// has its own stream and buffers, all freed when it returns (also when it fails).
// ---------------------------------------------------------------------------
// the checks before any device call: negative sizes, the bounds, then a missing array
static int cl_args(const char* who, int64_t n, int64_t nf, bool missing) {
    if (n < 0 || nf < 0) return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    if (n > cluster::kMaxItems)
        return set_err(MGP_E_INVALID, std::string(who) + ": more than 65536 items in one call (the distance matrix "
                                                         "is 8 n^2 bytes)");
    if (nf > cluster::kMaxFeat) return set_err(MGP_E_INVALID, std::string(who) + ": more than 2^24 features in one call");
    if (missing) return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    return MGP_OK;
}

// the `bad` word of the kernels, after the stream is idle
static int cl_bad(ClusterState& st, hipStream_t s, uint32_t* bad) {
    HIP_TRY(hipMemcpyAsync(bad, st.bad.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MGP_OK;
}

// st.dist [n][n] from the host's x [nf][n]; refuses a value that is not finite
static int cl_dist(ClusterState& st, hipStream_t s, const char* who, const double* x, int64_t n, int64_t nf) {
    MGP_TRY(st.dist.ensure((size_t)n * (size_t)n * 8));
    MGP_TRY(st.x.ensure(std::max<size_t>((size_t)n * (size_t)nf * 8, 8)));
    MGP_TRY(st.bad.ensure(4));
    if (nf) HIP_TRY(hipMemcpyAsync(st.x.p, x, (size_t)n * (size_t)nf * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(st.bad.p, 0, 4, s));
    VarProf prof(s);
    if (cluster::pair_dist(st.x.as<double>(), (int)n, (int)nf, st.dist.as<double>(), st.bad.as<uint32_t>(), s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": distance kernel launch failed");
    prof.stop();
    uint32_t bad = 0;
    MGP_TRY(cl_bad(st, s, &bad));
    prof.report(who, "items x features, pair distances", n, nf);
    if (bad) return set_err(MGP_E_INVALID, std::string(who) + ": a value of x is not finite");
    return MGP_OK;
}

// R's merge and order from the n - 1 raw steps (i < j, clusters named by their lowest member)
static void cl_tree(int64_t n, const int32_t* si, const int32_t* sj, int32_t* merge, int32_t* order) {
    std::vector<int32_t> lab((size_t)n);
    for (int64_t k = 0; k < n; ++k) lab[(size_t)k] = -(int32_t)(k + 1);
    for (int64_t s = 0; s + 1 < n; ++s) {
        int32_t a = lab[(size_t)si[s]], b = lab[(size_t)sj[s]];
        // a singleton before a cluster; two singletons by item (i < j); two clusters by step
        if ((a > 0 && b < 0) || (a > 0 && b > 0 && b < a)) std::swap(a, b);
        merge[2 * s] = a;
        merge[2 * s + 1] = b;
        lab[(size_t)si[s]] = (int32_t)(s + 1);
    }
    // the last merge's pair, every cluster replaced in place by its own pair: depth first, left to right
    std::vector<int32_t> stack;
    int64_t out = 0;
    if (n == 1) order[out++] = 1;
    if (n >= 2) stack.push_back((int32_t)(n - 1));
    while (!stack.empty()) {
        const int32_t e = stack.back();
        stack.pop_back();
        if (e < 0) {
            order[out++] = -e;
        } else {
            stack.push_back(merge[2 * (e - 1) + 1]);
            stack.push_back(merge[2 * (e - 1)]);
        }
    }
}

// the linkage on st.dist (overwritten), then merge / height / order on the host
static int cl_link(ClusterState& st, hipStream_t s, const char* who, int64_t n, int32_t* merge, double* height,
                   int32_t* order) {
    std::vector<int32_t> si((size_t)std::max<int64_t>(n - 1, 0)), sj(si.size());
    if (n >= 2) {
        MGP_TRY(st.nn.ensure((size_t)n * 4));
        MGP_TRY(st.dnn.ensure((size_t)n * 8));
        MGP_TRY(st.act.ensure((size_t)n));
        MGP_TRY(st.list.ensure((size_t)n * 4));
        MGP_TRY(st.si.ensure((size_t)n * 4));
        MGP_TRY(st.sj.ensure((size_t)n * 4));
        MGP_TRY(st.sh.ensure((size_t)n * 8));
        VarProf prof(s);
        if (cluster::linkage(st.dist.as<double>(), (int)n, st.nn.as<int32_t>(), st.dnn.as<double>(), st.act.as<uint8_t>(),
                             st.list.as<int32_t>(), st.si.as<int32_t>(), st.sj.as<int32_t>(), st.sh.as<double>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": linkage kernel launch failed");
        prof.stop();
        HIP_TRY(hipMemcpyAsync(si.data(), st.si.p, (size_t)(n - 1) * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(sj.data(), st.sj.p, (size_t)(n - 1) * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(height, st.sh.p, (size_t)(n - 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        prof.report(who, "items, linkage steps", n, n - 1);
        for (int64_t k = 0; k + 1 < n; ++k)
            if (si[(size_t)k] < 0 || sj[(size_t)k] <= si[(size_t)k] || sj[(size_t)k] >= n)
                return set_err(MGP_E_HIP, std::string(who) + ": the linkage returned an invalid step");
    }
    cl_tree(n, si.data(), sj.data(), merge, order);
    return MGP_OK;
}

int mgp_pair_dist(int device, const double* x, int64_t n_items, int64_t n_feat, double* out_dist) {
    const char* who = "mgp_pair_dist";
    MGP_TRY(cl_args(who, n_items, n_feat, n_items > 0 && (!out_dist || (n_feat > 0 && !x))));
    if (n_items == 0) return MGP_OK;
    return cl_call(device, [&](ClusterState& st, hipStream_t s) {
        MGP_TRY(cl_dist(st, s, who, x, n_items, n_feat));
        HIP_TRY(hipMemcpyAsync(out_dist, st.dist.p, (size_t)n_items * (size_t)n_items * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return (int)MGP_OK;
    });
}

int mgp_hclust_dist(int device, const double* dist, int64_t n_items, int32_t* merge, double* height, int32_t* order) {
    const char* who = "mgp_hclust_dist";
    MGP_TRY(cl_args(who, n_items, 0, (n_items > 0 && (!dist || !order)) || (n_items > 1 && (!merge || !height))));
    if (n_items == 0) return MGP_OK;
    return cl_call(device, [&](ClusterState& st, hipStream_t s) {
        const size_t bytes = (size_t)n_items * (size_t)n_items * 8;
        MGP_TRY(st.dist.ensure(bytes));
        MGP_TRY(st.bad.ensure(4));
        HIP_TRY(hipMemcpyAsync(st.dist.p, dist, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(st.bad.p, 0, 4, s));
        if (cluster::check_dist(st.dist.as<double>(), (int)n_items, st.bad.as<uint32_t>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": check kernel launch failed");
        uint32_t bad = 0;
        MGP_TRY(cl_bad(st, s, &bad));
        if (bad & cluster::BAD_VALUE)
            return set_err(MGP_E_INVALID, std::string(who) + ": a distance is negative or not finite");
        if (bad) return set_err(MGP_E_INVALID, std::string(who) + ": the distance matrix is not symmetric");
        return cl_link(st, s, who, n_items, merge, height, order);
    });
}

int mgp_hclust(int device, const double* x, int64_t n_items, int64_t n_feat, int32_t* merge, double* height,
               int32_t* order, double* out_dist) {
    const char* who = "mgp_hclust";
    MGP_TRY(cl_args(who, n_items, n_feat,
                    (n_items > 0 && (!order || (n_feat > 0 && !x))) || (n_items > 1 && (!merge || !height))));
    if (n_items == 0) return MGP_OK;
    return cl_call(device, [&](ClusterState& st, hipStream_t s) {
        MGP_TRY(cl_dist(st, s, who, x, n_items, n_feat));
        if (out_dist)  // (before the linkage overwrites the matrix)
            HIP_TRY(hipMemcpyAsync(out_dist, st.dist.p, (size_t)n_items * (size_t)n_items * 8, hipMemcpyDeviceToHost, s));
        return cl_link(st, s, who, n_items, merge, height, order);
    });
}

// ---------------------------------------------------------------------------
// mgp_knn / mgp_snn: the cells' k-nearest-neighbour graph over the heteroplasmy matrix's
// columns and Seurat's shared-nearest-neighbour graph of it (Signac's FindClonotypes ->
// FindNeighbors, the vignette's "Integration with Seurat/Signac"). No engine context, as the
// clustering: a call has its own stream and buffers, all freed when it returns.
// ---------------------------------------------------------------------------
// the checks before any device call that the two share: the sizes, then k against them
static int gr_args(const char* who, int64_t n, int64_t nf, int32_t k) {
    if (n < 0 || nf < 0) return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    if (n > graph::kMaxItems) return set_err(MGP_E_INVALID, std::string(who) + ": more than 2^20 items in one call");
    if (nf > graph::kMaxFeat) return set_err(MGP_E_INVALID, std::string(who) + ": more than 2^24 features in one call");
    if (k < 1 || k > graph::kMaxK)
        return set_err(MGP_E_INVALID, std::string(who) + ": k must be in 1..64 (a row's list is one entry per lane)");
    if (n > 0 && k > n - 1)
        return set_err(MGP_E_INVALID, std::string(who) + ": k must be at most n_items - 1 (an item is not its own "
                                                         "neighbour)");
    return MGP_OK;
}

static int gr_bad(GraphState& st, hipStream_t s, uint32_t* bad) {
    HIP_TRY(hipMemcpyAsync(bad, st.bad.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MGP_OK;
}

int mgp_knn(int device, const double* x, int64_t n_items, int64_t n_feat, int32_t k, int32_t* out_idx,
            double* out_dist) {
    const char* who = "mgp_knn";
    MGP_TRY(gr_args(who, n_items, n_feat, k));
    if (n_items > 0 && (!out_idx || !out_dist || (n_feat > 0 && !x)))
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    if (n_items == 0) return MGP_OK;
    const char* env = std::getenv("MGP_KNN_SPLITS");  // the candidate splits (0 or unset: automatic)
    const int splits = graph::knn_splits((int)n_items, env ? std::atoi(env) : 0);
    return cl_call<GraphState>(device, [&](GraphState& st, hipStream_t s) {
        const size_t n = (size_t)n_items, nk = n * (size_t)k;
        MGP_TRY(st.x.ensure(std::max<size_t>(n * (size_t)n_feat * 8, 8)));
        MGP_TRY(st.bad.ensure(4));
        MGP_TRY(st.part_dist.ensure((size_t)splits * nk * 8));
        MGP_TRY(st.part_idx.ensure((size_t)splits * nk * 4));
        MGP_TRY(st.out_dist.ensure(nk * 8));
        MGP_TRY(st.out_idx.ensure(nk * 4));
        if (n_feat) HIP_TRY(hipMemcpyAsync(st.x.p, x, n * (size_t)n_feat * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(st.bad.p, 0, 4, s));
        VarProf prof(s);
        if (graph::knn(st.x.as<double>(), (int)n_items, (int)n_feat, k, splits, st.part_dist.as<double>(),
                       st.part_idx.as<int32_t>(), st.out_dist.as<double>(), st.out_idx.as<int32_t>(),
                       st.bad.as<uint32_t>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
        prof.stop();
        uint32_t bad = 0;
        MGP_TRY(gr_bad(st, s, &bad));
        prof.report(who, (std::string("items x features, kNN, splits ") + std::to_string(splits)).c_str(), n_items,
                    n_feat);
        if (bad) return set_err(MGP_E_INVALID, std::string(who) + ": a value of x is not finite");
        HIP_TRY(hipMemcpyAsync(out_dist, st.out_dist.p, nk * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(out_idx, st.out_idx.p, nk * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return (int)MGP_OK;
    });
}

int mgp_snn(int device, const int32_t* knn_idx, int64_t n_items, int32_t k, int32_t min_shared, int64_t capacity,
            int64_t* n_edges, int32_t* out_i, int32_t* out_j, int32_t* out_shared) {
    const char* who = "mgp_snn";
    if (n_edges) *n_edges = 0;
    MGP_TRY(gr_args(who, n_items, 0, k));
    if (min_shared < 1 || min_shared > k + 1)
        return set_err(MGP_E_INVALID, std::string(who) + ": min_shared must be in 1..k + 1");
    if (!n_edges || capacity < 0 || (n_items > 0 && !knn_idx) || (capacity > 0 && (!out_i || !out_j || !out_shared)))
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    if (n_items == 0) return MGP_OK;
    return cl_call<GraphState>(device, [&](GraphState& st, hipStream_t s) {
        const int n = (int)n_items;
        const size_t un = (size_t)n_items, nk = un * (size_t)k, nkk = un * (size_t)(k + 1);
        MGP_TRY(st.idx.ensure(nk * 4));
        MGP_TRY(st.bad.ensure(4));
        HIP_TRY(hipMemcpyAsync(st.idx.p, knn_idx, nk * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(st.bad.p, 0, 4, s));
        VarProf check(s);
        if (graph::knn_check(st.idx.as<int32_t>(), n, k, st.bad.as<uint32_t>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": check kernel launch failed");
        check.stop();
        uint32_t bad = 0;
        MGP_TRY(gr_bad(st, s, &bad));
        check.report(who, "items x k, table check", n_items, k);
        if (bad)
            return set_err(MGP_E_INVALID, std::string(who) + ": the kNN table has an entry out of range, a row that "
                                                             "names itself or a repeated entry");
        MGP_TRY(st.sets.ensure(nkk * 4));
        MGP_TRY(st.deg.ensure(un * 4));
        MGP_TRY(st.off.ensure((un + 1) * 8));
        MGP_TRY(st.cur.ensure(un * 4));
        MGP_TRY(st.rev.ensure(nkk * 4));
        MGP_TRY(st.cnt.ensure(un * 4));
        MGP_TRY(st.eoff.ensure((un + 1) * 8));
        const int32_t* sets = st.sets.as<int32_t>();
        const int64_t* off = st.off.as<int64_t>();
        VarProf csr(s);
        if (graph::snn_sets(st.idx.as<int32_t>(), n, k, st.sets.as<int32_t>(), st.deg.as<int32_t>(), s) != 0 ||
            graph::scan(st.deg.as<int32_t>(), n, st.off.as<int64_t>(), s) != 0 ||
            graph::snn_reverse(sets, n, k, off, st.cur.as<int32_t>(), st.rev.as<int32_t>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": CSR kernel launch failed");
        csr.stop();
        VarProf count(s);
        if (graph::snn_edges(sets, n, k, off, st.rev.as<int32_t>(), min_shared, st.cnt.as<int32_t>(), nullptr, nullptr,
                             nullptr, nullptr, s) != 0 ||
            graph::scan(st.cnt.as<int32_t>(), n, st.eoff.as<int64_t>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": count kernel launch failed");
        count.stop();
        int64_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, st.eoff.as<int64_t>() + un, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        csr.report(who, "items x k, sorted sets and reverse lists", n_items, k);
        count.report(who, "items, edges, count pass", n_items, total);
        *n_edges = total;
        if (total > graph::kMaxEdges)
            return set_err(MGP_E_INVALID, std::string(who) + ": " + std::to_string(total) + " edges, more than 2^30 in "
                           "one call (a block of identical items gives a dense block: the output is then quadratic "
                           "in its size)");
        if (total > capacity)
            return set_err(MGP_E_INVALID, std::string(who) + ": " + std::to_string(total) + " edges, capacity " +
                                              std::to_string(capacity));
        if (total == 0) return (int)MGP_OK;
        const size_t ne = (size_t)total;
        MGP_TRY(st.ei.ensure(ne * 4));
        MGP_TRY(st.ej.ensure(ne * 4));
        MGP_TRY(st.es.ensure(ne * 4));
        VarProf fill(s);
        if (graph::snn_edges(sets, n, k, off, st.rev.as<int32_t>(), min_shared, nullptr, st.eoff.as<int64_t>(),
                             st.ei.as<int32_t>(), st.ej.as<int32_t>(), st.es.as<int32_t>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": fill kernel launch failed");
        fill.stop();
        HIP_TRY(hipMemcpyAsync(out_i, st.ei.p, ne * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(out_j, st.ej.p, ne * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(out_shared, st.es.p, ne * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        fill.report(who, "items, edges, fill pass", n_items, total);
        return (int)MGP_OK;
    });
}

// an integer threshold from the environment, read at call time: unset or not in lo..hi gives dflt
static int lv_env(const char* name, int lo, int hi, int dflt) {
    const char* e = std::getenv(name);
    if (!e || !*e) return dflt;
    const long v = std::strtol(e, nullptr, 10);
    return v < lo || v > hi ? dflt : (int)v;
}

// ---------------------------------------------------------------------------
// mgp_rank_sums: per feature (a row of x) the items sorted once, then every group's doubled
// midrank sum, its count of values > 0 and the row's tie term (mgp_rank.h): the integers of the
// Wilcoxon rank-sum test of each variant, a group against the rest (Seurat's FindAllMarkers on
// the alleles assay). No engine context, as the graphs. The features go in batches that keep
// the call's device memory under rank::kBudget; the results do not depend on the batch.
// ---------------------------------------------------------------------------
int mgp_rank_sums(int device, const double* x, int64_t n_items, int64_t n_feat, const int32_t* group, int32_t n_groups,
                  uint64_t* out_r2, uint32_t* out_pos, uint64_t* out_ties) {
    const char* who = "mgp_rank_sums";
    if (n_items < 0 || n_feat < 0) return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    if (n_items > rank::kMaxItems) return set_err(MGP_E_INVALID, std::string(who) + ": more than 2^20 items in one call");
    if (n_feat > rank::kMaxFeat) return set_err(MGP_E_INVALID, std::string(who) + ": more than 2^24 features in one call");
    if (n_groups < 1 || n_groups > rank::kMaxGroups)
        return set_err(MGP_E_INVALID, std::string(who) + ": n_groups must be in 1..65536");
    if ((n_feat > 0 && (!out_r2 || !out_pos || !out_ties)) || (n_items > 0 && !group) ||
        (n_items > 0 && n_feat > 0 && !x))
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    const size_t nf = (size_t)n_feat, ng = (size_t)n_groups;
    if (n_items == 0 || n_feat == 0) {  // nothing is ranked: every sum is 0
        if (nf) {
            std::fill(out_r2, out_r2 + nf * ng, (uint64_t)0);
            std::fill(out_pos, out_pos + nf * ng, (uint32_t)0);
            std::fill(out_ties, out_ties + nf, (uint64_t)0);
        }
        return MGP_OK;
    }
    const int tile = rank::tile_of(lv_env("MGP_RANK_TILE", rank::kMinTile, rank::kMaxTile, rank::kMaxTile));
    const int64_t batch = rank::batch_features(n_items, n_feat, n_groups, lv_env("MGP_RANK_BATCH", 0, 1 << 24, 0));
    return cl_call<RankState>(device, [&](RankState& st, hipStream_t s) {
        const size_t n = (size_t)n_items, P = (size_t)rank::padded(n_items), rows = (size_t)batch;
        MGP_TRY(st.group.ensure(n * 4));
        MGP_TRY(st.bad.ensure(4));
        MGP_TRY(st.x.ensure(rows * n * 8));
        MGP_TRY(st.keys.ensure(rows * P * 8));
        MGP_TRY(st.pay.ensure(rows * P * 4));
        MGP_TRY(st.r2.ensure(rows * ng * 8));
        MGP_TRY(st.pos.ensure(rows * ng * 4));
        MGP_TRY(st.ties.ensure(rows * 8));
        uint32_t bad = 0;
        auto fetch_bad = [&]() -> int {
            HIP_TRY(hipMemcpyAsync(&bad, st.bad.p, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            return MGP_OK;
        };
        // the labels first: no kernel indexes by one before they are known to be in range
        HIP_TRY(hipMemcpyAsync(st.group.p, group, n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(st.bad.p, 0, 4, s));
        if (rank::check_labels(st.group.as<int32_t>(), (int)n_items, n_groups, st.bad.as<uint32_t>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
        MGP_TRY(fetch_bad());
        if (bad) return set_err(MGP_E_INVALID, std::string(who) + ": a group label is outside 0 .. n_groups - 1");
        float kernel_ms = 0;
        for (size_t f0 = 0; f0 < nf; f0 += rows) {
            const size_t b = std::min(rows, nf - f0);
            HIP_TRY(hipMemcpyAsync(st.x.p, x + f0 * n, b * n * 8, hipMemcpyHostToDevice, s));
            VarProf prof(s);
            if (rank::sums(st.x.as<double>(), st.group.as<int32_t>(), (int)n_items, (int64_t)b, n_groups, tile,
                           st.keys.as<uint64_t>(), st.pay.as<uint32_t>(), st.r2.as<uint64_t>(), st.pos.as<uint32_t>(),
                           st.ties.as<uint64_t>(), st.bad.as<uint32_t>(), s) != 0)
                return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
            prof.stop();
            MGP_TRY(fetch_bad());
            kernel_ms += prof.ms();
            if (bad) return set_err(MGP_E_INVALID, std::string(who) + ": a value of x is not finite");
            HIP_TRY(hipMemcpyAsync(out_r2 + f0 * ng, st.r2.p, b * ng * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(out_pos + f0 * ng, st.pos.p, b * ng * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(out_ties + f0, st.ties.p, b * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (std::getenv("MGP_VAR_PROF"))
            std::fprintf(stderr, "[%s] %lld x %lld items x features, %d groups, tile %d, batch %lld: kernels %.3f ms\n", who,
                         (long long)n_items, (long long)n_feat, (int)n_groups, tile, (long long)batch, kernel_ms);
        return (int)MGP_OK;
    });
}

// ---------------------------------------------------------------------------
// mgp_sym_eig / mgp_pca: the eigenpairs of a symmetric matrix by the fixed-order Jacobi iteration of
// mgp_pca.h, and the principal components of the heteroplasmy matrix's columns with it (R's
// prcomp(t(af)), the vignette's "dimensionality reduction"). No engine context, as the graphs: a
// call has its own stream and buffers, all freed when it returns. Per sweep only the "rotated" word
// comes back; the eigenvalues are put in order here (a stable sort of m numbers), everything else
// runs on the device.
// ---------------------------------------------------------------------------
// the eigenpairs of st.a[0] [m][m] (overwritten): out_eig [m] descending (ties: the lower diagonal
// place first), st.vec [k][m] the first k vectors with the sign rule applied, *out_sweeps
static int pca_eig(PcaState& st, hipStream_t s, const char* who, int m, int k, double* out_eig, int32_t* out_sweeps) {
    const size_t mm = (size_t)m * (size_t)m;
    MGP_TRY(st.a[1].ensure(mm * 8));
    MGP_TRY(st.v[0].ensure(mm * 8));
    MGP_TRY(st.v[1].ensure(mm * 8));
    MGP_TRY(st.vec.ensure((size_t)k * (size_t)m * 8));
    MGP_TRY(st.perm.ensure((size_t)m * 4));
    MGP_TRY(st.bad.ensure(4));
    MGP_TRY(st.maxabs.ensure(8));
    MGP_TRY(st.flag.ensure(4));
    HIP_TRY(hipMemsetAsync(st.bad.p, 0, 4, s));
    HIP_TRY(hipMemsetAsync(st.maxabs.p, 0, 8, s));
    if (pca::sym_check(st.a[0].as<double>(), m, st.bad.as<uint32_t>(), st.maxabs.as<unsigned long long>(), s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": check kernel launch failed");
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, st.bad.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad & pca::BAD_VALUE) return set_err(MGP_E_INVALID, std::string(who) + ": a value of the matrix is not finite");
    if (bad) return set_err(MGP_E_INVALID, std::string(who) + ": the matrix is not symmetric");
    if (pca::identity(st.v[0].as<double>(), m, s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    int cur = 0, sweeps = 0;
    const int steps = m < 2 ? 0 : ((m + 1) & ~1) - 1;
    bool done = steps == 0;
    for (int sweep = 0; sweep < pca::kMaxSweeps && !done; ++sweep) {
        HIP_TRY(hipMemsetAsync(st.flag.p, 0, 4, s));
        for (int step = 0; step < steps; ++step, cur ^= 1)
            if (pca::jacobi_step(st.a[cur].as<double>(), st.v[cur].as<double>(), st.a[cur ^ 1].as<double>(),
                                 st.v[cur ^ 1].as<double>(), m, step, st.maxabs.as<unsigned long long>(),
                                 st.flag.as<uint32_t>(), s) != 0)
                return set_err(MGP_E_HIP, std::string(who) + ": Jacobi kernel launch failed");
        uint32_t rotated = 0;
        HIP_TRY(hipMemcpyAsync(&rotated, st.flag.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (rotated)
            ++sweeps;
        else
            done = true;
    }
    if (!done)
        return set_err(MGP_E_HIP, std::string(who) + ": the Jacobi iteration still rotated in sweep " +
                                      std::to_string(pca::kMaxSweeps) + " (no result is returned)");
    std::vector<double> diag((size_t)m);
    HIP_TRY(hipMemcpy2DAsync(diag.data(), 8, st.a[cur].p, ((size_t)m + 1) * 8, 8, (size_t)m, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<int32_t> perm((size_t)m);
    for (int i = 0; i < m; ++i) {
        perm[(size_t)i] = i;
        if (!(std::abs(diag[(size_t)i]) <= 1.7976931348623157e308))
            return set_err(MGP_E_INVALID, std::string(who) + ": the iteration overflowed (entries too large)");
    }
    std::stable_sort(perm.begin(), perm.end(),
                     [&](int32_t x, int32_t y) { return diag[(size_t)x] > diag[(size_t)y]; });
    for (int c = 0; c < m; ++c) out_eig[c] = diag[(size_t)perm[(size_t)c]];
    HIP_TRY(hipMemcpyAsync(st.perm.p, perm.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (perm is this frame's)
    if (pca::order_vectors(st.v[cur].as<double>(), st.perm.as<int32_t>(), m, k, st.vec.as<double>(), s) != 0)
        return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
    *out_sweeps = sweeps;
    return MGP_OK;
}

int mgp_sym_eig(int device, const double* a, int64_t m, double* out_eig, double* out_vec, int32_t* out_sweeps) {
    const char* who = "mgp_sym_eig";
    if (m < 0) return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    if (m > pca::kMaxFeat) return set_err(MGP_E_INVALID, std::string(who) + ": more than 2048 features in one call");
    if (!out_sweeps || (m > 0 && (!a || !out_eig || !out_vec)))
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    *out_sweeps = 0;
    if (m == 0) return MGP_OK;
    return cl_call<PcaState>(device, [&](PcaState& st, hipStream_t s) {
        const size_t mm = (size_t)m * (size_t)m;
        MGP_TRY(st.a[0].ensure(mm * 8));
        HIP_TRY(hipMemcpyAsync(st.a[0].p, a, mm * 8, hipMemcpyHostToDevice, s));
        VarProf prof(s);
        MGP_TRY(pca_eig(st, s, who, (int)m, (int)m, out_eig, out_sweeps));
        prof.stop();
        HIP_TRY(hipMemcpyAsync(out_vec, st.vec.p, mm * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        prof.report(who, (std::string("rows x sweeps, Jacobi")).c_str(), m, *out_sweeps);
        return (int)MGP_OK;
    });
}

int mgp_pca(int device, const double* x, int64_t n_items, int64_t n_feat, int32_t scale, int32_t n_comp,
            double* out_mean, double* out_sd, double* out_eig, double* out_loadings, double* out_scores,
            double* out_cov, int32_t* out_sweeps) {
    const char* who = "mgp_pca";
    if (n_items < 0 || n_feat < 0) return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    if (n_items > pca::kMaxItems) return set_err(MGP_E_INVALID, std::string(who) + ": more than 2^20 items in one call");
    if (n_feat > pca::kMaxFeat) return set_err(MGP_E_INVALID, std::string(who) + ": more than 2048 features in one call");
    if (n_items < 2) return set_err(MGP_E_INVALID, std::string(who) + ": at least 2 items are needed");
    if (n_comp < 1) return set_err(MGP_E_INVALID, std::string(who) + ": n_comp must be at least 1");
    if (n_comp > std::min(n_feat, n_items - 1))
        return set_err(MGP_E_INVALID, std::string(who) + ": n_comp must be at most min(n_feat, n_items - 1)");
    if (!x || !out_mean || (scale && !out_sd) || !out_eig || !out_loadings || !out_scores || !out_sweeps)
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    *out_sweeps = 0;
    const int tile = pca::cov_tile((int)n_feat, lv_env("MGP_PCA_TILE", 16, 64, 0));  // (changes no result)
    return cl_call<PcaState>(device, [&](PcaState& st, hipStream_t s) {
        const int n = (int)n_items, m = (int)n_feat, k = n_comp, S = pca::slabs(n_items);
        const size_t un = (size_t)n, um = (size_t)m, mm = um * um;
        MGP_TRY(st.x.ensure(un * um * 8));
        MGP_TRY(st.z.ensure(un * um * 8));
        MGP_TRY(st.part.ensure((size_t)S * um * 8));
        MGP_TRY(st.mean.ensure(um * 8));
        MGP_TRY(st.var.ensure(um * 8));
        MGP_TRY(st.sd.ensure(um * 8));
        MGP_TRY(st.covp.ensure((size_t)S * mm * 8));
        MGP_TRY(st.cov.ensure(mm * 8));
        MGP_TRY(st.a[0].ensure(mm * 8));
        MGP_TRY(st.scores.ensure((size_t)k * un * 8));
        MGP_TRY(st.bad.ensure(4));
        HIP_TRY(hipMemcpyAsync(st.x.p, x, un * um * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(st.bad.p, 0, 4, s));
        const double *dx = st.x.as<double>(), *mean = st.mean.as<double>();
        const double* sd = scale ? st.sd.as<double>() : nullptr;
        VarProf p_mean(s);
        if (pca::slab_sums(dx, nullptr, n, m, st.part.as<double>(), st.bad.as<uint32_t>(), s) != 0 ||
            pca::slab_reduce(st.part.as<double>(), m, S, (double)n, st.mean.as<double>(), nullptr, s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
        uint32_t bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, st.bad.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (bad) return set_err(MGP_E_INVALID, std::string(who) + ": a value of x is not finite");
        if (scale && (pca::slab_sums(dx, mean, n, m, st.part.as<double>(), st.bad.as<uint32_t>(), s) != 0 ||
                      pca::slab_reduce(st.part.as<double>(), m, S, (double)(n - 1), st.var.as<double>(),
                                       st.sd.as<double>(), s) != 0))
            return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
        if (pca::standardize(dx, mean, sd, n, m, st.z.as<double>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": kernel launch failed");
        p_mean.stop();
        VarProf p_cov(s);
        if (pca::covariance(st.z.as<double>(), n, m, tile, st.covp.as<double>(), st.cov.as<double>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": covariance kernel launch failed");
        p_cov.stop();
        HIP_TRY(hipMemcpyAsync(st.a[0].p, st.cov.p, mm * 8, hipMemcpyDeviceToDevice, s));
        VarProf p_eig(s);
        MGP_TRY(pca_eig(st, s, who, m, k, out_eig, out_sweeps));
        p_eig.stop();
        VarProf p_sc(s);
        if (pca::scores(st.z.as<double>(), st.vec.as<double>(), n, m, k, st.scores.as<double>(), s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": scores kernel launch failed");
        p_sc.stop();
        HIP_TRY(hipMemcpyAsync(out_mean, st.mean.p, um * 8, hipMemcpyDeviceToHost, s));
        if (scale) {
            HIP_TRY(hipMemcpyAsync(out_sd, st.sd.p, um * 8, hipMemcpyDeviceToHost, s));
        } else if (out_sd) {  // the covariance's diagonal, its square root taken below
            HIP_TRY(hipMemcpy2DAsync(out_sd, 8, st.cov.p, (um + 1) * 8, 8, um, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipMemcpyAsync(out_loadings, st.vec.p, (size_t)k * um * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(out_scores, st.scores.p, (size_t)k * un * 8, hipMemcpyDeviceToHost, s));
        if (out_cov) HIP_TRY(hipMemcpyAsync(out_cov, st.cov.p, mm * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!scale && out_sd)
            for (size_t f = 0; f < um; ++f) out_sd[f] = std::sqrt(out_sd[f]);
        p_mean.report(who, "items x features, means and scaling", n_items, n_feat);
        p_cov.report(who, (std::string("items x features, covariance, tile ") + std::to_string(tile)).c_str(), n_items,
                     n_feat);
        p_eig.report(who, "features x sweeps, Jacobi", n_feat, *out_sweeps);
        p_sc.report(who, "items x components, scores", n_items, n_comp);
        return (int)MGP_OK;
    });
}

// ---------------------------------------------------------------------------
// mgp_louvain: the communities of an integer-weighted graph, the cells' clonotypes when the graph
// is mgp_snn's (Signac's FindClonotypes -> FindClusters). The definition is pinned in
// include/mgpileup.h; the loop of levels and passes runs here, and per pass only the moved
// count, the bad word, I and the partial sums of tot^2 come back. No engine context, as the graphs.
// ---------------------------------------------------------------------------
// S = double(M2) * double(I) - gamma * double(B): two products and a difference, each rounded on
// its own; the conversion of the 128-bit B is the compiler's correctly rounded one
static double lv_score(uint64_t m2, uint64_t internal, unsigned __int128 b, double gamma) {
#pragma clang fp contract(off)
    const double x = (double)m2 * (double)internal;
    const double y = gamma * (double)b;
    return x - y;
}

int mgp_louvain(int device, int64_t n_vertices, int64_t n_edges, const int32_t* edge_i, const int32_t* edge_j,
                const int32_t* edge_w, double resolution, int32_t max_levels, int32_t max_passes, int32_t* labels,
                int64_t* n_communities, double* modularity, uint64_t* sums, int32_t* n_levels, int64_t* levels) {
    const char* who = "mgp_louvain";
    if (n_communities) *n_communities = 0;
    if (n_levels) *n_levels = 0;
    if (n_vertices < 0 || n_edges < 0 || !n_communities || !modularity || !sums || !n_levels || !levels ||
        (n_vertices > 0 && !labels) || (n_edges > 0 && (!edge_i || !edge_j || !edge_w)))
        return set_err(MGP_E_INVALID, std::string(who) + ": bad arguments");
    if (n_vertices > louvain::kMaxVertices)
        return set_err(MGP_E_INVALID, std::string(who) + ": more than 2^20 vertices in one call");
    if (n_edges > louvain::kMaxEdges)
        return set_err(MGP_E_INVALID, std::string(who) + ": more than 2^30 edges in one call");
    if (!(resolution > 0.0) || !(resolution <= 1.7976931348623157e308))
        return set_err(MGP_E_INVALID, std::string(who) + ": the resolution must be finite and above 0");
    if (max_levels < 1 || max_levels > louvain::kMaxLevels)
        return set_err(MGP_E_INVALID, std::string(who) + ": max_levels must be in 1..64");
    if (max_passes < 1 || max_passes > louvain::kMaxPasses)
        return set_err(MGP_E_INVALID, std::string(who) + ": max_passes must be in 1..65536");
    if (n_edges > 0 && n_vertices < 2)
        return set_err(MGP_E_INVALID, std::string(who) + ": an edge needs two vertices");
    *modularity = 0.0;
    sums[0] = sums[1] = sums[2] = sums[3] = 0;
    if (n_edges == 0) {  // nothing is launched: every vertex its own community
        for (int64_t v = 0; v < n_vertices; ++v) labels[v] = (int32_t)v;
        *n_communities = n_vertices;
        return MGP_OK;
    }
    // the move kernel's thresholds (rows up to the first: a wave; up to the second: the LDS table)
    const int wave_row = lv_env("MGP_LOUVAIN_WAVE_ROW", 0, louvain::kWaveRow, louvain::kWaveRow);
    const int lds_row = lv_env("MGP_LOUVAIN_LDS_ROW", 0, louvain::kLdsRow, louvain::kLdsRow);
    return cl_call<LouvainState>(device, [&](LouvainState& st, hipStream_t s) {
        using namespace louvain;
        const int n0 = (int)n_vertices;
        const size_t un = (size_t)n_vertices, ne = (size_t)n_edges, m0 = 2 * ne;
        const size_t res_bytes = 16 + (size_t)kScoreBlocks * 16;  // moved, bad, I, the (hi, lo) pairs
        for (DevBuf* b : {&st.ei, &st.ej, &st.wq}) MGP_TRY(b->ensure(ne * 4));
        MGP_TRY(st.res.ensure(res_bytes));
        for (DevBuf* b : {&st.deg, &st.cur, &st.c, &st.next, &st.list_mid, &st.list_long, &st.flag, &st.map})
            MGP_TRY(b->ensure(un * 4));
        for (DevBuf* b : {&st.tot, &st.tot_next, &st.cap, &st.d[0], &st.d[1], &st.self[0], &st.self[1]})
            MGP_TRY(b->ensure(un * 8));
        for (DevBuf* b : {&st.ren, &st.slot, &st.off[0], &st.off[1]}) MGP_TRY(b->ensure((un + 1) * 8));
        MGP_TRY(st.counts.ensure(8));
        for (int k = 0; k < 2; ++k) {
            MGP_TRY(st.nbr[k].ensure(m0 * 4));
            MGP_TRY(st.src[k].ensure(m0 * 4));
            MGP_TRY(st.w[k].ensure(m0 * 8));
        }
        MGP_TRY(st.tkeys.ensure(2 * m0 * 4));
        MGP_TRY(st.tvals.ensure(2 * m0 * 8));
        int32_t* moved = st.res.as<int32_t>();
        uint32_t* bad = st.res.as<uint32_t>() + 1;
        uint64_t* internal = st.res.as<uint64_t>() + 1;
        uint64_t* partial = st.res.as<uint64_t>() + 2;
        Csr g[2];
        for (int k = 0; k < 2; ++k)
            g[k] = Csr{st.off[k].as<int64_t>(), st.nbr[k].as<int32_t>(), st.src[k].as<int32_t>(), st.w[k].as<uint64_t>()};
        HIP_TRY(hipMemcpyAsync(st.ei.p, edge_i, ne * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(st.ej.p, edge_j, ne * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(st.wq.p, edge_w, ne * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(st.res.p, 0, res_bytes, s));
        std::vector<int32_t> iota(un);
        for (size_t v = 0; v < un; ++v) iota[v] = (int32_t)v;
        HIP_TRY(hipMemcpyAsync(st.map.p, iota.data(), un * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(st.self[0].p, 0, un * 8, s));

        // ---- build: the checks, the degrees, the symmetric CSR, the repeated pairs
        VarProf build(s);
        if (build_degrees(st.ei.as<int32_t>(), st.ej.as<int32_t>(), st.wq.as<int32_t>(), n_edges, n0,
                          st.deg.as<int32_t>(), st.d[0].as<uint64_t>(), bad, s) != 0 ||
            scan32(st.deg.as<int32_t>(), n0, g[0].off, s) != 0 ||
            build_fill(st.ei.as<int32_t>(), st.ej.as<int32_t>(), st.wq.as<int32_t>(), n_edges, n0, st.cur.as<int32_t>(),
                       g[0], s) != 0 ||
            build_repeats(g[0], (int64_t)m0, st.tkeys.as<int32_t>(), bad, s) != 0)
            return set_err(MGP_E_HIP, std::string(who) + ": build kernel launch failed");
        build.stop();
        std::vector<uint64_t> res(res_bytes / 8);
        const auto fetch = [&]() -> int {
            HIP_TRY(hipMemcpyAsync(res.data(), st.res.p, res_bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            return MGP_OK;
        };
        const auto res_bad = [&]() { return (uint32_t)(res[0] >> 32); };
        const auto res_moved = [&]() { return (int64_t)(res[0] & 0xFFFFFFFFu); };
        const auto res_b = [&]() {
            unsigned __int128 b = 0;
            for (int k = 0; k < kScoreBlocks; ++k) b += ((unsigned __int128)res[2 + 2 * k] << 64) | res[3 + 2 * k];
            return b;
        };
        MGP_TRY(fetch());
        build.report(who, "vertices, edges, build", n_vertices, n_edges);
        if (res_bad() & BAD_EDGE)
            return set_err(MGP_E_INVALID, std::string(who) + ": an edge is not i < j with both in [0, n_vertices)");
        if (res_bad() & BAD_WEIGHT)
            return set_err(MGP_E_INVALID, std::string(who) + ": a weight is outside 1..2^20");
        if (res_bad() & BAD_REPEAT) return set_err(MGP_E_INVALID, std::string(who) + ": a pair is repeated");
        if (res_bad()) return set_err(MGP_E_HIP, std::string(who) + ": a table overflowed in the build");
        uint64_t m2 = 0;
        for (size_t e = 0; e < ne; ++e) m2 += 2 * (uint64_t)edge_w[e];

        // ---- the levels
        VarProf run(s);
        int cur = 0, nl = n0, n_lv = 0;
        int64_t m = (int64_t)m0, total_passes = 0;
        uint64_t best_i = 0;
        unsigned __int128 best_b = 0;
        int32_t *c = st.c.as<int32_t>(), *next = st.next.as<int32_t>();
        uint64_t *tot = st.tot.as<uint64_t>(), *tot_next = st.tot_next.as<uint64_t>();
        while (true) {
            const uint64_t* d = st.d[cur].as<uint64_t>();
            const uint64_t* self = st.self[cur].as<uint64_t>();
            int32_t counts[2] = {0, 0};
            if (level_start(g[cur], nl, d, c, tot, wave_row, lds_row, st.list_mid.as<int32_t>(),
                            st.list_long.as<int32_t>(), st.counts.as<int32_t>(), s) != 0 ||
                score(g[cur], m, nl, c, self, tot, internal, partial, s) != 0)
                return set_err(MGP_E_HIP, std::string(who) + ": level kernel launch failed");
            HIP_TRY(hipMemcpyAsync(counts, st.counts.p, 8, hipMemcpyDeviceToHost, s));
            MGP_TRY(fetch());
            best_i = res[1];
            best_b = res_b();
            double best = lv_score(m2, best_i, best_b, resolution);
            int passes = 0, accepted = 0, undone = 0;
            while (passes < max_passes && undone < 2) {
                HIP_TRY(hipMemcpyAsync(next, c, (size_t)nl * 4, hipMemcpyDeviceToDevice, s));
                if (move(g[cur], nl, c, tot, d, m2, resolution, passes & 1, wave_row, st.list_mid.as<int32_t>(),
                         counts[0], st.list_long.as<int32_t>(), counts[1], st.tkeys.as<int32_t>(),
                         st.tvals.as<uint64_t>(), next, bad, s) != 0 ||
                    apply(nl, c, next, d, tot_next, moved, s) != 0 ||
                    score(g[cur], m, nl, next, self, tot_next, internal, partial, s) != 0)
                    return set_err(MGP_E_HIP, std::string(who) + ": pass kernel launch failed");
                MGP_TRY(fetch());
                if (res_bad()) return set_err(MGP_E_HIP, std::string(who) + ": a community table overflowed");
                ++passes;
                const unsigned __int128 b = res_b();
                const double sc = lv_score(m2, res[1], b, resolution);
                if (res_moved() > 0 && sc > best) {  // accepted: the new labels and totals are the level's
                    std::swap(c, next);
                    std::swap(tot, tot_next);
                    best = sc, best_i = res[1], best_b = b;
                    ++accepted;
                    undone = 0;
                } else {
                    ++undone;  // undone: the labels and totals stay as they were
                }
            }
            total_passes += passes;
            // ---- the non-empty communities, in label order, are the next level's vertices
            int64_t n2 = 0;
            if (agg_flag(nl, c, st.flag.as<int32_t>(), s) != 0 ||
                scan32(st.flag.as<int32_t>(), nl, st.ren.as<int64_t>(), s) != 0 ||
                agg_map(n0, st.map.as<int32_t>(), c, st.ren.as<int64_t>(), s) != 0)
                return set_err(MGP_E_HIP, std::string(who) + ": renumbering kernel launch failed");
            HIP_TRY(hipMemcpyAsync(&n2, st.ren.as<int64_t>() + nl, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            levels[4 * n_lv + 0] = nl, levels[4 * n_lv + 1] = n2, levels[4 * n_lv + 2] = passes,
                              levels[4 * n_lv + 3] = accepted;
            ++n_lv;
            if (n2 == nl || n2 == 1 || n_lv >= max_levels) break;
            const int nx = cur ^ 1;
            int64_t m_next = 0;
            if (agg_vertices(g[cur], m, nl, (int)n2, c, st.ren.as<int64_t>(), st.flag.as<int32_t>(), tot, self,
                             st.d[nx].as<uint64_t>(), st.self[nx].as<uint64_t>(), st.cap.as<int64_t>(), s) != 0 ||
                scan64(st.cap.as<int64_t>(), n2, st.slot.as<int64_t>(), s) != 0 ||
                agg_insert(g[cur], m, c, st.ren.as<int64_t>(), st.slot.as<int64_t>(), st.tkeys.as<int32_t>(),
                           st.tvals.as<uint64_t>(), bad, s) != 0 ||
                agg_rows((int)n2, st.slot.as<int64_t>(), st.tkeys.as<int32_t>(), st.tvals.as<uint64_t>(),
                         st.deg.as<int32_t>(), nullptr, s) != 0 ||
                scan32(st.deg.as<int32_t>(), n2, g[nx].off, s) != 0 ||
                agg_rows((int)n2, st.slot.as<int64_t>(), st.tkeys.as<int32_t>(), st.tvals.as<uint64_t>(), nullptr,
                         &g[nx], s) != 0)
                return set_err(MGP_E_HIP, std::string(who) + ": aggregation kernel launch failed");
            HIP_TRY(hipMemcpyAsync(&m_next, g[nx].off + n2, 8, hipMemcpyDeviceToHost, s));
            MGP_TRY(fetch());
            if (res_bad()) return set_err(MGP_E_HIP, std::string(who) + ": a coarse row's table overflowed");
            cur = nx, nl = (int)n2, m = m_next;
        }
        run.stop();
        std::vector<int32_t> raw(un);
        HIP_TRY(hipMemcpyAsync(raw.data(), st.map.p, un * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        run.report(who, "levels, passes", n_lv, total_passes);
        // numbered from 0 by descending size, ties by smallest member
        const size_t nc = (size_t)levels[4 * (n_lv - 1) + 1];
        std::vector<int64_t> size(nc, 0), first(nc, -1);
        for (size_t v = 0; v < un; ++v) {
            const size_t r = (size_t)raw[v];
            if (r >= nc) return set_err(MGP_E_HIP, std::string(who) + ": a label out of range");
            if (size[r]++ == 0) first[r] = (int64_t)v;
        }
        std::vector<int32_t> order(nc), rank(nc);
        for (size_t r = 0; r < nc; ++r) order[r] = (int32_t)r;
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            return size[a] != size[b] ? size[a] > size[b] : first[a] < first[b];
        });
        for (size_t k = 0; k < nc; ++k) rank[(size_t)order[k]] = (int32_t)k;
        for (size_t v = 0; v < un; ++v) labels[v] = rank[(size_t)raw[v]];
        *n_communities = (int64_t)nc;
        *n_levels = n_lv;
        sums[0] = m2, sums[1] = best_i, sums[2] = (uint64_t)(best_b >> 64), sums[3] = (uint64_t)best_b;
        *modularity = lv_score(m2, best_i, best_b, resolution) / (double)m2 / (double)m2;
        return (int)MGP_OK;
    });
}

}  // extern "C"
