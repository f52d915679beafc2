// dml_host.h — what the host translation units of the C-ABI share (dml_store*.hip,
// dml_prereduce.hip, dml_group.hip). Host only; the types the kernels see are in
// dml_internal.h. Not part of the public ABI.
#pragma once
#include "distml_ps.h"
#include "dml_internal.h"

#include <string>

// Returns DML_E_HIP from the calling function, with the failing expression and HIP's
// message as the thread's dml_last_error().
#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess)                                                                      \
            return dml::set_error(DML_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_));      \
    } while (0)

namespace dml {

// Device push pointers are 4-byte aligned (include/distml_ps.h): every kernel reads keys
// as dwords and values with 4-byte-aligned 16-B loads. The entry points that take device
// pushes refuse anything else, like a null pointer, before they launch, change state or
// join a collective (dml_shard_split, dml_split.hip, checks the same way).
inline constexpr const char* kMisalignedPush = "device push pointer is not 4-byte aligned";
static inline bool push_ptrs_aligned(const void* const* bufs, int n) {
    for (int i = 0; i < n; ++i)
        if ((uintptr_t)bufs[i] & 3u) return false;
    return true;
}

namespace {  // per translation unit, like the static helpers here: nothing of this header is exported
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};
}  // namespace

// Workspaces of a store's pipeline and of a pre-reduce context: a ring of kRing, at most
// kRing-1 chunks pending: chunk j's index reuses chunk j-3's workspace, whose Ctrl chunk
// j-2 read as `prev` — and chunk j-2 has been retired before chunk j launches.
constexpr int kRing = 3;

// DataDesc keySize / valueSize (DataDesc.java:50-51) and a dense matrix record's stride.
static inline int desc_key_bytes(const dml_desc& d) { return d.key_type == 0 ? 4 : 8; }
static inline int desc_value_bytes(const dml_desc& d) { return d.value_type == DML_ELEMENT_TYPE_DOUBLE ? 8 : 4; }
static inline int64_t desc_row_stride(const dml_desc& d, int32_t cols) {
    return desc_key_bytes(d) + (int64_t)desc_value_bytes(d) * cols;
}

// Full-range pushes: at least one, and every push lists `rows` records.
static inline bool all_full_range(const Batch& bt, int nb, int64_t rows) {
    for (int j = 0; j < nb; ++j)
        if (bt.nrec[j] != rows) return false;
    return nb > 0;
}
// Full-range pushes whose slot table is beyond the caches: rows x slot_stride(nb) x 4 B above
// `min_bytes`. There the index's slot atomics go to DRAM, and a complete key check
// (k_ident_full) ahead of it pays (see prereduce_begin_tail, dml_prereduce.hip).
constexpr int64_t kIdentFullMinBytes = (int64_t)64 << 20;
static inline bool full_range_beyond_caches(const Batch& bt, int nb, int64_t rows, int64_t min_bytes) {
    return rows * slot_stride(nb) * 4 > min_bytes && all_full_range(bt, nb, rows);
}

// The pushes of a chunk whose speculation was verified (Ctrl::spec_ok), counted as identity,
// reused (slots read from a kept column) or indexed. Returns the slot-table columns that now
// hold a verified permutation (indexed or reused, not identity): Workspace::perm.
static inline uint64_t tally_verified_pushes(const Ctrl& h, int nb, dml_store_counters& st) {
    uint64_t perm = 0;
    for (int b = 0; b < nb; ++b) {
        if (ctrl_identity(&h, h.ident, b)) {
            st.identity_pushes += 1;
            continue;
        }
        if ((h.ident >> b) & 1ull) st.reused_pushes += 1;
        else st.indexed_pushes += 1;
        perm |= 1ull << ctrl_col(&h, b);
    }
    return perm;
}
// The pushes of a chunk that did not speculate: identity where a complete key check
// (Batch::ident_ok) let them skip the index, indexed otherwise.
static inline void tally_checked_pushes(const Ctrl& h, int nb, bool ident_ok, dml_store_counters& st) {
    for (int b = 0; b < nb; ++b) {
        if (ident_ok && ((h.ident >> b) & 1ull)) st.identity_pushes += 1;
        else st.indexed_pushes += 1;
    }
}

}  // namespace dml
