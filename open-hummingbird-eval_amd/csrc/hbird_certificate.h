// The bounds behind the certificate of the fp16 screen (use_fp16 and the automatic state), as plain C++ without HIP types: the
// re-rank kernels call them on the device (hbird_rerank_dev.h), hb_certificate_bound_replay on the host (hbird_calibrate.cpp) -- the CPU tests
// that hold "E is a bound" on the adversarial worlds evaluate THESE constants.
// The kernels' unit contracts floating-point expressions into FMAs and which ones depends on the expressions' shape: operand order and
// parentheses below are part of the result.
#pragma once
#include <math.h>

#ifdef __HIP__
#define HB_HD __host__ __device__
#else
#define HB_HD
#endif

// both inputs of a product rounded to fp16: relative 2^-10 per product (with 5 % to spare), Cauchy-Schwarz over the row
constexpr float HB_CERT_F16 = 1.05f / 1024.0f;

// E >= |fp16 score - exact score| of any row of a query (both inputs rounded to fp16: relative 2^-10 per product,
// Cauchy-Schwarz over the row; fp32 accumulation: D * 2^-23).  qn = ||q||, bmax = max ||b||.
// A non-finite E (query norm) skips nothing in the re-rank, and fails the certificate.
HB_HD inline float hb_certificate_bound(float qn, float bmax, int d, int metric) {
    return qn * bmax * (HB_CERT_F16 + (float)d * 2.4e-7f)
           + (qn + bmax) * sqrtf((float)d) * 6e-8f                 // fp16 subnormal inputs
           + (metric == 1 ? (float)d * 1.2e-7f * 0.5f * bmax * bmax : 0.0f)  // |row init| in the sums
           + 1e-30f;
}

// The centred pass' bound E' >= |pass score + c_q - exact score| (derivation: DESIGN.md 4).  qc = ||fl(q - t mu)||, cmax = max ||fl(b - mu)||,
// qn = ||q||, bmax = max ||b||, mun = ||mu||, at = |t|; D' = D + 4 pays for the fmaf of init16 and the additions of the comparison itself.
HB_HD inline float hb_certificate_bound_centred(float qc, float cmax, float mun, float at, float qn, float bmax, int d, int metric) {
    const float du = (float)(d + 4) * 1.2e-7f;
    return qc * cmax * (HB_CERT_F16 + du)                                                          // fp16 images of both centred operands; the pass' fp32 sums
           + du * (qn * bmax + qn * mun + 2.0f * at * mun * cmax + (metric == 1 ? bmax * bmax : 0.0f))   // exact chain; chain of c_q; chain of g, init16 and its share of the sums; |row init|
           + (qc + cmax) * sqrtf((float)d) * 6e-8f                                                 // fp16 subnormal inputs
           + 1e-30f;
}
