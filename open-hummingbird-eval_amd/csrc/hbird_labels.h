// The label table of an index: its own rows (fp32 values, or uint16 counts j of values j / P), the counters that describe them, the sticky
// flag of the conversion, and the table it may borrow instead (multi-GPU: all-gathered labels / norms covering a GLOBAL id range).
// Plain C++ over hbird_devbuf.h, no HIP, in the style of hbird_mirror.h -- data, questions, transitions: tests/labels_check.cpp drives the
// type on the host.  The HIP work stays with the callers (hbird_labels.hip, hbird_select.hip, hbird_aggregate.hip, hbird_grid.hip), who are
// handed the store's pointers: the conversion and gather launches, the flag's memset and read-back, and the stream synchronisation before
// anything that drops a buffer (hb_devbuf's contract; `*_drops` says whether a transition will).
//
// What holds between calls:
//   - at most ONE row buffer exists, the one of the current form (P == 0: fp32, P > 0: counts), and `cap` describes it: cap > 0 exactly
//     where it exists, in rows of the current width.  A change of form or of width therefore drops the buffer and the capacity together
//     (hb_index_reset keeps allocations: rows of another form or width may follow it).
//   - nrows <= cap, and nchecked <= nrows.
//   - `c`, the class count, is ONE number shared by own and borrowed rows: adding own rows sets it, and so does borrowing a table.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <utility>
#include "hbird_devbuf.h"

// The table one K5 launch reads (hbird_aggregate.hip, hbird_grid.hip), chosen in ONE place for all three kernels: label rows (fp32: P = 0) of
// stride ls covering the global ids [id_base, id_base + nlabels), norms covering [norm_base, norm_base + nnorm).  hb_label_store::view fills
// everything but `wide` (whether the 16-byte gather of count rows applies: hb_k5_table_choose, beside the kernels' K5_LUT).
struct hb_k5_table {
    const void* labels; bool u16; int P, ls; int64_t nlabels;
    const float* bnorm; int64_t norm_base, nnorm;
    int64_t id_base;
    int wide;
};

// what a question or transition of the store answers besides "fine"; the caller words the message (every entry has its own)
enum hb_label_status {
    HB_LABELS_OK = 0,
    HB_LABELS_FAILED = -1,          // an allocation or copy failed: hb_fail has the reason, the store is as it was
    HB_LABELS_ROWS_MISSING = 1,     // view: neither a borrowed table nor own rows for every bank row
    HB_LABELS_HOLD_ROWS = 2         // set_denominator: rows of another denominator are stored
};

struct hb_label_form { int c, P; };      // what adopt() replaces and restore() may put back

struct hb_label_store {
    hb_dev<float> rows32;           // [cap][c] fp32 (P == 0) ...
    hb_dev<uint16_t> rows16;        // ... or [cap][stride()] uint16 counts: rows padded to 8 counts = 16 B for K5's wide gather
    hb_dev<int> flag;               // sticky device flag: a label value was not a multiple of 1 / P (made by the first conversion)
    int c = 0, P = 0;
    int64_t nrows = 0, cap = 0;
    int64_t nchecked = 0;           // rows whose conversion has been read back (hb_labels_checked: one read-back after the table grew)
    // the borrowed table: dense [b_n][c] fp32 or counts of denominator b_P, with norms, covering the global ids [b_base, b_base + b_n)
    const float* b32 = nullptr; const uint16_t* b16 = nullptr; const float* b_norm = nullptr;
    int b_P = 0; int64_t b_n = 0, b_base = 0;

    // ---- questions
    int classes() const { return c; }
    int denominator() const { return P; }
    bool counts() const { return P > 0; }
    int stride() const { return P ? (c + 7) & ~7 : c; }                        // elements per stored row
    size_t row_bytes() const { return (size_t)stride() * (P ? 2 : 4); }
    int64_t rows() const { return nrows; }
    int64_t capacity() const { return cap; }
    bool allocated() const { return own_base<void>() != nullptr; }             // (rows may be none: an emptied index keeps its buffer)
    bool own_rows() const { return nrows > 0 && allocated(); }
    bool covers(int64_t ntotal) const { return allocated() && nrows >= ntotal; }
    bool borrowed() const { return b32 || b16; }
    bool missing(int64_t ntotal) const { return !borrowed() && !covers(ntotal); }
    int64_t unchecked() const { return P > 0 && flag && nchecked < nrows ? nrows - nchecked : 0; }
    // the stored rows and the place of the next one, read as T (float, uint16_t, or the 16-byte pieces of hb_index_add_from)
    template <class T> T* own_base() const { return static_cast<T*>(P ? rows16.p : rows32.p); }
    template <class T> T* own_tail() const { return reinterpret_cast<T*>(static_cast<char*>(P ? rows16.p : rows32.p) + (size_t)nrows * row_bytes()); }
    // The table of an aggregation on an index of ntotal rows with norms bnorm, asked with ids from id_base on: a borrowed table where there
    // is one, else the own rows; norms_all [n_all]: the label-sharded form, the own rows with everybody's norms.
    hb_label_status view(int64_t id_base, int64_t ntotal, const float* bnorm, const float* norms_all, int64_t n_all, hb_k5_table* t) const {
        t->u16 = counts(); t->labels = own_base<const void>(); t->P = P; t->ls = stride();
        t->nlabels = nrows; t->id_base = id_base;
        t->bnorm = bnorm; t->norm_base = id_base; t->nnorm = nrows;
        t->wide = 0;
        if (norms_all) {
            if (!covers(ntotal)) return HB_LABELS_ROWS_MISSING;
            t->nlabels = ntotal; t->bnorm = norms_all; t->norm_base = 0; t->nnorm = n_all;
        } else if (borrowed()) {
            t->ls = c;                                   // borrowed tables are dense [n, C]
            t->u16 = b16 != nullptr;
            t->labels = t->u16 ? (const void*)b16 : (const void*)b32; t->P = b_P;
            t->bnorm = b_norm; t->nlabels = t->nnorm = b_n; t->id_base = t->norm_base = b_base;
        } else if (!covers(ntotal)) return HB_LABELS_ROWS_MISSING;
        if (!t->u16) t->P = 0;
        return HB_LABELS_OK;
    }

    // ---- transitions (where `*_drops` says so, the caller has synchronised the stream first)
    void drop() { rows32.drop(); rows16.drop(); cap = 0; }
    // fp32 values <-> counts, or another denominator: refused while rows are stored; a change of form leaves no buffer of the old one
    bool set_denominator_drops(int newP) const { return (newP == 0) != (P == 0) && allocated(); }
    hb_label_status set_denominator(int newP) {
        if (nrows > 0 && newP != P) return HB_LABELS_HOLD_ROWS;
        if (set_denominator_drops(newP)) drop();
        P = newP;
        return HB_LABELS_OK;
    }
    // Room for n_more rows of c_new classes: a buffer of another width goes (its capacity counts rows of the OLD width, so it does even where
    // `cap` rows would seem to fit); the kept rows move with a growth, whose capacity follows the bank's, else grows x 1.5.  Sets c.
    bool ensure_drops(int c_new) const { return c_new != c && cap > 0; }
    hb_label_status ensure(int c_new, int64_t n_more, int64_t bank_cap, void* stream) {
        set_width(c_new);
        if (nrows + n_more <= cap) return HB_LABELS_OK;
        const int64_t new_cap = std::max<int64_t>(nrows + n_more, std::max<int64_t>(bank_cap, cap + cap / 2));
        hb_devbuf& table = P ? static_cast<hb_devbuf&>(rows16) : rows32;
        if (table.ensure_keep((size_t)new_cap * row_bytes(), HB_GROW_EXACT, (size_t)nrows * row_bytes(), stream)) return HB_LABELS_FAILED;
        cap = new_cap;
        return HB_LABELS_OK;
    }
    // n rows were written at own_tail(): converted from fp32 values (hb_index_add_labels: the flag speaks of them once it is read back), or
    // copied in their stored form (hb_index_add_from: what was valid in the source stays valid, so a table that was caught up still is)
    void appended(int64_t n, bool converted) {
        if (!converted && nchecked == nrows) nchecked = nrows + n;
        nrows += n;
    }
    void checked() { nchecked = nrows; }
    // hb_index_reset: no rows, nothing checked; the allocations stay.  -> the device flag the caller clears (nullptr: none yet)
    int* emptied() { nrows = 0; nchecked = 0; return flag; }
    // hb_index_labels_to_fp32: the count rows are replaced by `table`, their fp32 values in a buffer of cap_new rows (no rows: no buffer)
    int64_t fp32_capacity() const { return std::max<int64_t>(nrows, cap); }
    void replace_with_fp32(hb_dev<float>&& table, int64_t cap_new) {
        drop();
        cap = table ? cap_new : 0; rows32 = std::move(table); P = 0; nchecked = 0;
    }
    // A store without rows takes the class count and denominator of the rows about to be copied in (hb_index_add_from into an empty index,
    // hb_index_select_rows); -> the form it had.  restore(old) after a failing ensure: a store that is left without a buffer is given its
    // form back, one that kept a buffer keeps the new form.
    hb_label_form form() const { return {c, P}; }
    bool adopt_drops(int c_new, int newP) const { return set_denominator_drops(newP) || ensure_drops(c_new); }
    hb_label_form adopt(int c_new, int newP) {
        const hb_label_form old = form();
        if (set_denominator(newP) == HB_LABELS_OK) set_width(c_new);
        return old;
    }
    void restore(hb_label_form old) {
        if (nrows == 0 && !allocated()) { c = old.c; P = old.P; }
    }
    // a table of n dense rows of c_new classes with their norms, for the global ids [id_base, id_base + n): sets c; replaces what was borrowed
    void borrow_f32(const float* labels, const float* bnorm, int64_t n, int c_new, int64_t id_base) {
        b32 = labels; b16 = nullptr; b_P = 0; b_norm = bnorm; b_n = n; b_base = id_base; c = c_new;
    }
    void borrow_counts(const uint16_t* counts_, const float* bnorm, int64_t n, int c_new, int P_, int64_t id_base) {
        b32 = nullptr; b16 = counts_; b_P = P_; b_norm = bnorm; b_n = n; b_base = id_base; c = c_new;
    }
    void unborrow() { b32 = nullptr; b16 = nullptr; b_P = 0; b_norm = nullptr; b_n = 0; b_base = 0; }      // (c stays)

private:
    void set_width(int c_new) {
        if (ensure_drops(c_new)) drop();
        c = c_new;
    }
};
