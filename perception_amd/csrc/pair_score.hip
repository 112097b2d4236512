// pair_score.hip - the two-way registration score (rule C21, k_pair_score.hip): the step of the fused batch call, the context's
// setting, the read-back of the per-cluster scores, one pair as a call of its own and the rule as a host call
#include <numeric>

#include "context.hpp"

namespace {
// Scores `np` pairs into out[0 .. np): the pairs that step 8 lets through become two jobs each (source -> template, template ->
// source), their items go to the device largest first, one launch on the context's stream fills the integer rows (step 3's tau:
// tau_of), one blocking copy brings them back and pair_record writes the records.  May grow its buffers (which synchronises the
// stream); ends synchronised.
int run_pair_scores(cd_context* c, const std::vector<ResultSpec>& specs, double max_range, double min_cov, double min_inl, cd_pair_score* out) {
    const int np = (int)specs.size();
    if (np <= 0) return CD_OK;
    std::vector<int> pre((size_t)np);
    std::vector<PairJob> jobs;
    std::vector<PairItem> items;
    std::vector<long long> weight;
    for (int k = 0; k < np; ++k) {
        const ResultSpec& s = specs[(size_t)k];
        const int m = s.slot >= 0 && s.slot < CD_MAX_TEMPLATES ? c->tpl_m[s.slot] : 0;
        pre[(size_t)k] = pair_pre_status(s.n, m, s.T);
        if (pre[(size_t)k] != CD_OK) continue;
        if (s.src_off < 0 || s.src_off + s.n > 0x7fffffffll) return fail(c, CD_ERR_CAPACITY, "a cluster's points lie beyond 2^31 records");
        for (int dir = 0; dir < 2; ++dir) {
            PairJob j;
            std::memset(&j, 0, sizeof(j));
            j.q_src = dir == 0;
            j.q_off = dir == 0 ? (int32_t)s.src_off : c->tpl_off[s.slot]; j.nq = dir == 0 ? s.n : m;
            j.g_off = dir == 0 ? c->tpl_off[s.slot] : (int32_t)s.src_off; j.ng = dir == 0 ? m : s.n;
            j.pair = k;
            std::memcpy(j.T, s.T, sizeof(j.T));
            // the job's queries in equal chunks of at most PS_CHUNK
            const int chunks = (j.nq + PS_CHUNK - 1) / PS_CHUNK, each = (j.nq + chunks - 1) / chunks;
            for (int q0 = 0; q0 < j.nq; q0 += each) {
                items.push_back(PairItem{(int32_t)jobs.size(), q0, std::min(each, j.nq - q0), 0});
                weight.push_back((long long)items.back().qn * j.ng);
            }
            jobs.push_back(j);
        }
    }
    const int n_items = (int)items.size();
    std::vector<unsigned long long> acc((size_t)np * PAIR_ACC_PITCH, 0ull);
    if (n_items > 0) {
        std::vector<int> order((size_t)n_items);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return weight[(size_t)a] > weight[(size_t)b]; });
        const size_t acc_words = (size_t)np * PAIR_ACC_PITCH + PAIR_ACC_PITCH;   // (the queue word behind the rows)
        GROW(c, d_psjob, jobs.size()); GROW(c, h_psjob, jobs.size());
        GROW(c, d_psitem, items.size()); GROW(c, h_psitem, items.size());
        GROW(c, d_psacc, acc_words); GROW(c, h_psacc, acc_words);
        std::memcpy(c->h_psjob.get(), jobs.data(), sizeof(PairJob) * jobs.size());
        for (int i = 0; i < n_items; ++i) c->h_psitem[i] = items[(size_t)order[(size_t)i]];
        HIPCHK(c, hipMemcpyAsync(c->d_psjob, c->h_psjob, sizeof(PairJob) * jobs.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_psitem, c->h_psitem, sizeof(PairItem) * items.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_psacc, 0, sizeof(unsigned long long) * acc_words, c->stream));
        int* queue = reinterpret_cast<int*>(c->d_psacc.get() + (size_t)np * PAIR_ACC_PITCH);
        LAUNCH(c, launch_pair_score(c->stream, n_items, 4 * std::max(c->n_cu, 1), c->d_psjob, c->d_psitem, c->d_src0, c->d_tpl, tau_of(max_range), c->d_psacc, queue));
        HIPCHK(c, copy_sync(c, c->h_psacc, c->d_psacc, sizeof(unsigned long long) * (size_t)np * PAIR_ACC_PITCH, hipMemcpyDeviceToHost));
        std::memcpy(acc.data(), c->h_psacc.get(), sizeof(unsigned long long) * acc.size());
    }
    for (int k = 0; k < np; ++k) {
        const ResultSpec& s = specs[(size_t)k];
        const int m = s.slot >= 0 && s.slot < CD_MAX_TEMPLATES ? c->tpl_m[s.slot] : 0;
        const unsigned long long* row = acc.data() + (size_t)k * PAIR_ACC_PITCH;
        if (pre[(size_t)k] == CD_OK && row[PAIR_BAD] == 0ull && (row[PAIR_N_SRC_IN] > (unsigned long long)s.n || row[PAIR_N_TPL_IN] > (unsigned long long)m))
            return fail(c, CD_ERR_DEVICE, "the pair-score kernel left an inconsistent row");
        pair_record(s.n, m, pre[(size_t)k], row, s.accepted, min_cov, min_inl, &out[k]);
    }
    return CD_OK;
}

int pair_score_points_impl(cd_context* c, int slot, const void* src_xyz, size_t stride, int n, const float* T, double max_range, double min_cov,
                           double min_inl, int accepted, cd_pair_score* out) {
    invalidate_last(c);
    if (int st = check_result_points(c, out != nullptr, slot, src_xyz, stride, n, T, pair_thresholds_ok(max_range, min_cov, min_inl),
                                     "max_range must be finite and > 0, the fractions in [0, 1]"))
        return st;
    if (int st = upload_points(c, src_xyz, stride, n, c->d_src0)) return st;
    const std::vector<ResultSpec> one{ResultSpec{0, n, slot, accepted ? 1 : 0, T}};
    return run_pair_scores(c, one, max_range, min_cov, min_inl, out);
}
}  // namespace

namespace cd {
// The fused call's step between its ICP (every stage synchronised, c->last_clusters final) and publish_last.
// in: the clusters' points as extracted, d_src0 + orig_off[k] (size of the result), the templates in d_tpl, every result's T,
// template_slot and accepted.  out: last_pair, one record per cluster (not valid before publish_last).
int stage_pair_scores(cd_context* c, int ncl, const std::vector<long long>& orig_off) {
    c->last_pair.begin(ncl);
    if (ncl <= 0) return CD_OK;
    std::vector<cd_pair_score> rec((size_t)ncl);
    if (int st = run_pair_scores(c, result_specs(c, ncl, orig_off), c->pair_range, c->pair_min_cov, c->pair_min_inl, rec.data())) return st;
    for (int k = 0; k < ncl; ++k) c->last_pair.keep(k, rec[(size_t)k]);
    return CD_OK;
}
}  // namespace cd

extern "C" {
int cd_set_pair_score(cd_context* c, int enable, double max_range, double min_coverage, double min_inlier_fraction) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (!pair_thresholds_ok(max_range, min_coverage, min_inlier_fraction)) return fail(c, CD_ERR_INVALID_ARG, "max_range must be finite and > 0, the fractions in [0, 1]");
    c->pair_on = enable ? 1 : 0;
    c->pair_range = max_range;
    c->pair_min_cov = min_coverage;
    c->pair_min_inl = min_inlier_fraction;
    return CD_OK;
}

int cd_get_pair_score(const cd_context* c, int* enable, double* max_range, double* min_coverage, double* min_inlier_fraction) {
    if (!c) return CD_ERR_INVALID_ARG;
    if (enable) *enable = c->pair_on;
    if (max_range) *max_range = c->pair_range;
    if (min_coverage) *min_coverage = c->pair_min_cov;
    if (min_inlier_fraction) *min_inlier_fraction = c->pair_min_inl;
    return CD_OK;
}

int cd_pair_score_struct_size(void) { return (int)sizeof(cd_pair_score); }

int cd_get_cluster_pair_scores(const cd_context* c, int frame, int first, int count, cd_pair_score* out) {
    return c ? c->last_pair.read(frame, first, count, out) : CD_ERR_INVALID_ARG;
}

int cd_pair_score_points(cd_context* c, int slot, const void* src_xyz, size_t stride_bytes, int n, const float T[16], double max_range, double min_coverage,
                         double min_inlier_fraction, int accepted, cd_pair_score* out) {
    return with_scan_retry(c, [&] { return pair_score_points_impl(c, slot, src_xyz, stride_bytes, n, T, max_range, min_coverage, min_inlier_fraction, accepted, out); });
}

int cd_pair_score_host(const void* tpl_xyz, size_t tpl_stride, int m, const void* src_xyz, size_t src_stride, int n, const float T[16], double max_range,
                       double min_coverage, double min_inlier_fraction, int accepted, cd_pair_score* out) {
    if (!out || !T || m < 0 || n < 0 || (m > 0 && !tpl_xyz) || (n > 0 && !src_xyz) || tpl_stride < 12 || src_stride < 12) return CD_ERR_INVALID_ARG;
    if (!pair_thresholds_ok(max_range, min_coverage, min_inlier_fraction)) return CD_ERR_INVALID_ARG;
    const int pre = pair_pre_status(n, m, T);
    unsigned long long acc[PAIR_ACC_PITCH] = {0ull};
    if (pre == CD_OK) {
        const std::vector<float> tpl = gather_xyz(tpl_xyz, tpl_stride, m), src = gather_xyz(src_xyz, src_stride, n);
        pair_passes_host(tpl.data(), m, src.data(), n, T, tau_of(max_range), acc);
    }
    pair_record(n, m, pre, acc, accepted ? 1 : 0, min_coverage, min_inlier_fraction, out);
    return CD_OK;
}
}  // extern "C"
