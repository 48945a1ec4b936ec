// What the two linear-probe units share (hbird_linprobe.hip, hbird_linprobe_class.hip): the parameters in the kernels' fragment layout and
// host launchers for the kernels of hbird_linprobe.hip that take any class-tile count -- the staged rows, the backward contraction, the
// float64 segment adds, the loss tree and the finish.  One definition each, so that the image-level probe's gradient cannot drift from the
// segmentation probe's bits.
#pragma once
#include "hbird_internal.h"

#define LP_THREADS 512
#define LP_ROWS 256                  // rows of a forward workgroup (eight waves x one 32-row tile)
#define LP_GC 8                      // column groups of Wb staged in LDS at a time (one KiB per class tile each)
#define LP_TREE_BLOCKS 256

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

// the parameters in the kernels' form: Wb [C][D + 1] -> wt [ct][g8][256] (the bank's fragment layout with classes as rows), bias [32 ct]
struct lp_params {
    hb_dev<float> wt, bias;
    int ct = 0;
    int make(const hb_index* ix, const float* Wb, int C, hipStream_t s);      // linprobe_retile_kernel
};

// Each launcher enqueues on `s` and returns 0, or -1 with hb_last_error set when the launch failed.
// linprobe_stage_rows_kernel: the chunk's rows row0 .. row0 + rows_pad - 1 as row-major [1, x, 0 ..] of stride xs; `skip` is indexed by bank row
int hb_lp_stage_rows(const hb_index* ix, int64_t row0, int64_t rows_pad, const unsigned char* skip, float* X, int xs, hipStream_t s);
// linprobe_backward_kernel: partial [nseg][32 ct][xs] from resid [rows_pad][32 ct] and X [rows_pad][xs]
int hb_lp_backward(int ct, const float* resid, const float* X, int xs, int64_t seg_rows, int64_t rows_pad, int nseg, float* partial, hipStream_t s);
// linprobe_reduce_kernel: grad [C][d1] float64 += the chunk's segment partials in ascending segment order
int hb_lp_reduce(const float* partial, int nseg, int cp, int xs, int C, int d1, double* grad, hipStream_t s);
// the loss tree: scal[0 .. 2] = {sum of the row losses, rows used, sum of Wb^2}; tree holds 2 LP_TREE_BLOCKS doubles
int hb_lp_loss_tree(const float* rowloss, const unsigned char* skip, int64_t n, double* tree, const float* Wb, int64_t total, double* scal, hipStream_t s);
// linprobe_finish_kernel: grad = grad / n + l2 Wb
int hb_lp_finish(double* grad, const float* Wb, int64_t total, double n, double l2, hipStream_t s);
// the workspace of a call in bytes: hb_linprobe_set_workspace's value, or HB_LINPROBE_WORKSPACE
int64_t hb_lp_workspace();
