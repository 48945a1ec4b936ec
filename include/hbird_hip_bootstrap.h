/* Part of the C ABI of libhbird_hip.so: paired bootstrap over images for mIoU grids (csrc/hbird_bootstrap.hip).
 * Stands on its own (no hb_index_t): hbird_hip.h does not include it, hbird_mi/_lib.py binds it as SIGNATURES_BOOTSTRAP.
 * Every pointer is a device pointer, every call enqueues on `stream` (NULL: the default stream) and returns 0, or -1 with hb_last_error set
 * before anything is launched.
 *
 * Per-image class counts.  A pixel counts iff !(has_ignore && gt == ignore) && 0 <= gt < G && 0 <= pred < G (hb_confusion_update's rule
 * with P = G).  A counted pixel with pred == gt: tp[gt] += 1; with pred != gt: fp[pred] += 1 and fn[gt] += 1.  One image gives 3 G int32
 * values [G][3] = (tp, fp, fn).  Summed over images this is the identity matching (PredsmIoU.compute(linear_probe=True)) of the total
 * confusion matrix.
 * hb_image_class_counts: gt, pred [B][h][w] int64; image b's block is WRITTEN (not accumulated) at out + b * row_stride (int32 elements,
 * row_stride >= 3 G); nothing outside the B blocks is touched.  h * w < 2^31.
 *
 * The stats table: stats[n_img][cols] int32, cols = n_cfg * 3 G, image-major -- one image's blocks of every configuration are contiguous.
 *
 * Resampler.  splitmix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 * return z ^ z >> 31 (uint64).  draw(seed, r, j) = mulhi64(splitmix(splitmix(seed) + (r << 32) + j), N), the high 64 bits of the 128-bit
 * product, 0 <= r < 2^20, 0 <= j < N.  W[r][i] = #{j : draw(seed, r, j) == i}: every row sums to N.  The draws depend on (seed, r, j, N)
 * only -- not on the configurations, not on how R is cut into chunks -- so replicates are paired across columns.  The multiply-high
 * reduction is biased by at most N / 2^64 per value; not corrected.
 * hb_bootstrap_multiplicities: out[R][n_img] int32 = rows r0 .. r0 + R - 1 of W.  1 <= n_img <= HB_BOOTSTRAP_MAX_IMAGES, r0 + R <= 2^20.
 *
 * hb_bootstrap_counts: out[r][col] = sum_i W[r][i] * stats[i][col] in int64, exact.  W[R][n_img] int32, out[R][cols] int64.
 *
 * hb_bootstrap_miou: m[r][c] = (sum_{g ascending} tp / max(tp + fp + fn, 1e-8)) / G in float64, sequentially, of the replicate counts of
 * configuration c; out_samples[R][n_cfg], and out_point[n_cfg] the same with W == 1.  Replicates run in chunks whose workspace (W and
 * the int64 counts) stays within 256 MiB; chunk_replicates > 0 sets the chunk (tests), 0 = automatic.  The results do not depend on it.
 * Returns after the stream has finished (the workspace is local to the call). */
#ifndef HBIRD_HIP_BOOTSTRAP_H
#define HBIRD_HIP_BOOTSTRAP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define HB_BOOTSTRAP_MAX_IMAGES 32768
#define HB_BOOTSTRAP_MAX_REPLICATES 1048576
int hb_image_class_counts(const int64_t* gt, const int64_t* pred, int64_t B, int h, int w, int G, int64_t ignore, int has_ignore,
                          int32_t* out, int64_t row_stride, void* stream);
int hb_bootstrap_multiplicities(int n_img, uint64_t seed, int64_t r0, int64_t R, int32_t* out, void* stream);
int hb_bootstrap_counts(const int32_t* stats, int64_t n_img, int64_t cols, const int32_t* W, int64_t R, int64_t* out, void* stream);
int hb_bootstrap_miou(const int32_t* stats, int n_img, int n_cfg, int G, uint64_t seed, int64_t R, double* out_point,
                      double* out_samples, int64_t chunk_replicates, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* HBIRD_HIP_BOOTSTRAP_H */
