// The lazily kept copies of the bank (fp16 fragment tiles with their mean-centred side arrays, fp32 rows for the re-rank) and the one
// bookkeeping type they share.  Plain C++ over hbird_devbuf.h, no HIP: tests/mirror_check.cpp drives these types on the host.  The copies
// are made, converted and read by the searches (hbird_knn.hip, hbird_f16_centre.hip); hb_index::bank_changed tells them what happened to
// the bank.  A drop keeps hb_devbuf's contract: the caller has synchronised the stream where work may still read the buffer.
#pragma once
#include <stdint.h>
#include <utility>
#include "hbird_devbuf.h"

// What a copy knows about itself: three numbers, and the questions and transitions its users have.
struct hb_bank_mirror {
    int64_t cap = 0;                // the capacity (rows) the copy is allocated for; 0: no copy
    int64_t rows = 0;               // rows converted so far
    int64_t declined_cap = -1;      // the capacity at which the copy was found not to fit (not asked again per search); -1: never

    bool has(int64_t c) const { return cap != 0 && cap == c; }      // a copy for a bank of this capacity
    bool declined_at(int64_t c) const { return declined_cap == c; }
    bool behind(int64_t ntotal) const { return rows < ntotal; }
    // the 32-row tiles still to convert for a bank of ntotal rows: n_rt tiles from rt0 on (a partly filled last tile is converted again)
    void pending(int64_t ntotal, int64_t* rt0, int64_t* n_rt) const { *rt0 = rows / 32; *n_rt = (ntotal + 31) / 32 - *rt0; }

    void allocated(int64_t c) { cap = c; rows = 0; }
    void converted(int64_t ntotal) { rows = ntotal; }
    void declined(int64_t c) { declined_cap = c; }
    void ask_again() { declined_cap = -1; }
    void emptied() { rows = 0; }                 // the bank was emptied: the allocation and the declined mark belong to the capacity
    void dropped() { cap = 0; rows = 0; }
};

// The mean-centred form of the fp16 copy (hbird_f16_centre.hip).  Its row arrays are allocated for the copy's capacity and go with the copy;
// the rows converted with mu are the copy's own count while `active`.
struct hb_centre_state {
    hb_dev<float> mu;               // [max(dp16, dp)] column mean of the rows present when the copy was made (0 on the padding dimensions)
    hb_dev<float> g;                // [cap] mu.(b - mu), k-ascending fp32 chain
    hb_dev<float> init16;           // [cap] the candidate kernel's row init of the current search: fmaf(t, g, binit)
    hb_dev<float> sc;               // device scalars {cmax = max ||b - mu||, ||mu|| (rounded up), mu.mu, t of the last search}
    hb_dev<char> qaux;              // per search: [c_q nq][||q - t mu|| nq][partial sums of c_q]
    int active = 0;                 // the fp16 copy holds centred rows (0: no copy yet, or a non-finite / all-zero mean: the plain copy)
    // (whose queries' c_q and ||q - t mu|| lie in qaux, and of which level: the search's report, hbird_report.h)

    void drop() {
        mu.drop(); g.drop(); init16.drop(); sc.drop(); qaux.drop();
        active = 0;
    }
};

// The fp16 fragment tiles the candidate pass reads: [cap / 32][dp16 / 16][...] (hbird_knn_f16.hip), plain or centred.
struct hb_fp16_copy {
    hb_dev<void> tiles;
    hb_bank_mirror m;
    hb_dev<int> flag; int overflow = 0;      // sticky device flag and its host image: a finite bank value overflowed fp16, the fp32 kernel serves this bank
    hb_centre_state centre;

    // The tiles for a bank of `cap` rows of row_bytes each; what there was goes first.  quiet (the automatic state, where the copy only buys
    // speed): a failure is noted as "declined at cap" and reported to nobody; else it is the caller's error (hb_fail).  -> 0 / -1
    int make(int64_t cap, size_t row_bytes, bool quiet) {
        drop();
        const size_t need = (size_t)cap * row_bytes;
        if (quiet ? tiles.try_ensure(need, HB_GROW_EXACT) != nullptr : tiles.ensure(need, HB_GROW_EXACT) != 0) {
            if (quiet) m.declined(cap);
            return -1;
        }
        m.allocated(cap);
        return 0;
    }
    bool has_centre_arrays() const { return centre.mu && centre.g && centre.init16 && centre.sc; }
    // mu [n_mu], the two row arrays for the copy's capacity, the scalars.  Four locals until all are there: a failing allocation frees the
    // earlier ones and leaves the copy as it was.
    int make_centre_arrays(size_t n_mu) {
        hb_dev<float> mu, g, init16, sc;
        if (mu.ensure(n_mu * 4, HB_GROW_EXACT) || g.ensure((size_t)m.cap * 4, HB_GROW_EXACT) || init16.ensure((size_t)m.cap * 4, HB_GROW_EXACT) ||
            sc.ensure(16, HB_GROW_EXACT)) return -1;
        centre.drop();
        centre.mu = std::move(mu); centre.g = std::move(g); centre.init16 = std::move(init16); centre.sc = std::move(sc);
        return 0;
    }
    int64_t centred_rows() const { return centre.active ? m.rows : 0; }      // rows converted with mu

    void emptied() { m.emptied(); overflow = 0; }      // (the caller clears the device flag; a centred copy derives its mean anew: rows == 0)
    // the tiles go with the row arrays that were sized like them; mu, the scalars and `active` stay until the next conversion replaces them
    void drop() { tiles.drop(); centre.g.drop(); centre.init16.drop(); m.dropped(); }
    // ... and a change of the copy's form (hb_index_set_fp16_centre): everything, the overflow image and the declined mark included
    void drop_form() { drop(); centre.drop(); overflow = 0; m.ask_again(); }
};

// The bank once more as plain fp32 rows [row][rs] for the exact re-rank (hbird_knn_f16.hip), where memory allows.
struct hb_row_copy {
    hb_dev<float> rows;
    hb_bank_mirror m;
    int rs = 0;                     // floats per row

    bool has(int64_t cap, int stride) const { return rows && m.has(cap) && rs == stride; }
    // The copy for `cap` rows of `stride` floats.  A failing allocation reports nothing and leaves "declined at cap".  -> made or not
    bool make(int64_t cap, int stride) {
        drop();
        if (rows.try_ensure((size_t)cap * stride * 4, HB_GROW_EXACT)) { m.declined(cap); return false; }
        m.allocated(cap); m.ask_again(); rs = stride;
        return true;
    }
    int64_t bytes() const { return rows ? m.cap * (int64_t)rs * 4 : 0; }
    void drop() { rows.drop(); m.dropped(); }
};
