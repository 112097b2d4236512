// kept_records.hpp - the per-cluster records a context keeps of its last call for a read-back (cd_get_cluster_plane_stats,
// cd_get_cluster_coarse_stats, cd_get_cluster_reject_stats, cd_get_cluster_recip_stats, cd_get_cluster_pair_scores,
// cd_get_cluster_shape_frames): the records, frame-major, the index of every frame's first record in them (F + 1 entries) and
// whether a read may answer from them.  Host only, no HIP header and no context: batch.hip and cd_icp fill a table,
// invalidate_last clears it, the getters read it; kept_records_check.cpp runs it on a CPU (tests/test_kept_records_cpu.py).
#pragma once
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/cuboid_hip.h"

namespace cd {

template <class T>
class KeptRecords {
    static_assert(std::is_trivially_copyable<T>::value, "records are copied by bytes");
    std::vector<T> rec_;
    std::vector<int> first_;
    bool ok_ = false;

public:
    // a fused call starts its ICP part: max(ncl, 1) default records, not valid before publish (so a call that fails in between
    // leaves "nothing to read" rather than an old index into new records)
    void begin(int ncl) { rec_.assign((size_t)std::max(ncl, 1), T()); ok_ = false; }
    // record k <- one record of a stage's pinned mirror (S: the kernels' layout of T)
    template <class S>
    void keep(int k, const S& src) {
        static_assert(sizeof(S) == sizeof(T) && std::is_trivially_copyable<S>::value, "the mirror's record has the layout of the API's");
        std::memcpy(&rec_[(size_t)k], &src, sizeof(T));
    }
    // all n records of a stage at once (n = 0: none)
    template <class S>
    void assign_all(const S* src, int n) {
        static_assert(sizeof(S) == sizeof(T) && std::is_trivially_copyable<S>::value, "the mirror's record has the layout of the API's");
        rec_.resize((size_t)std::max(n, 0));
        if (n > 0) std::memcpy(rec_.data(), src, sizeof(T) * (size_t)n);
    }
    void publish(const std::vector<int>& first) { first_ = first; ok_ = true; }   // the index of every frame's first record (F + 1 entries)
    // a call over one problem (cd_icp): one frame, one record
    template <class S>
    void publish_single(const S& src) {
        rec_.assign(1, T());
        keep(0, src);
        first_.assign({0, 1});
        ok_ = true;
    }
    void invalidate() { ok_ = false; }
    bool valid() const { return ok_; }
    const T& operator[](size_t k) const { return rec_[k]; }

    // records first .. first + count of `frame` into out: the number written, or CD_ERR_INVALID_ARG - not valid (the mode off, the
    // call failed or another compute call has run since), a negative argument, no buffer to write to, no such frame, or an index that
    // does not describe the records
    int read(int frame, int first, int count, T* out) const {
        if (!ok_ || frame < 0 || first < 0 || count < 0 || (count > 0 && !out)) return CD_ERR_INVALID_ARG;
        if ((size_t)frame + 1 >= first_.size()) return CD_ERR_INVALID_ARG;
        const int lo = first_[(size_t)frame], hi = first_[(size_t)frame + 1];
        if (lo < 0 || hi < lo || (size_t)hi > rec_.size()) return CD_ERR_INVALID_ARG;
        int n = 0;
        for (long long k = (long long)lo + first; k < hi && n < count; ++k) out[n++] = rec_[(size_t)k];
        return n;
    }
};

}  // namespace cd
