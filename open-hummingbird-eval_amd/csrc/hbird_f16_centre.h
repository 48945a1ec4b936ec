// The mean-centred form of the fp16 candidate copy (hbird_f16_centre.hip): state kept per index, and what the re-rank kernels take of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "hbird_devbuf.h"

struct hb_index;

struct hb_centre_state {
    hb_dev<float> mu;               // [max(dp16, dp)] column mean of the rows present when the copy was made (0 on the padding dimensions)
    hb_dev<float> g;                // [cap_rows] mu.(b - mu), k-ascending fp32 chain
    hb_dev<float> init16;           // [cap_rows] the candidate kernel's row init of the current search: fmaf(t, g, binit)
    hb_dev<float> sc;               // device scalars {cmax = max ||b - mu||, ||mu|| (rounded up), mu.mu, t of the last search}
    hb_dev<char> qaux;              // per search: [c_q nq][||q - t mu|| nq][partial sums of c_q]
    int64_t cap_rows = 0;           // capacity the row arrays were allocated for
    int64_t rows = 0;               // rows converted with mu
    int active = 0;                 // the fp16 copy holds centred rows (0: no copy yet, or a non-finite / all-zero mean: the plain copy)
    // hb_index_last_centre: host bookkeeping of the last centred pass (hb_centre_queries), whose c_q and ||q - t mu|| lie in qaux
    int64_t q_n = 0;                // its queries
    int q_level = -1;               // 0: a caller's pass, 1: the second pass over its uncertified queries, -1: none since the state was dropped
};

// per-query constants of one centred pass, for the re-rank: c_q = q.mu, ||q - t mu||, the device scalars above
struct hb_centre_view { const float* cq; const float* qcn; const float* sc; };

void hb_centre_drop(hb_index* ix);
int hb_centre_convert(hb_index* ix, hipStream_t s, int* centred_out);
int hb_centre_queries(hb_index* ix, int64_t nq, int first, _Float16* q16, hb_centre_view* view, hipStream_t s);
int hb_centre_readout(hb_index* ix, float* mu, float* scalars, float* g, float* init16, uint16_t* bank16, float* cq, float* qcn, uint16_t* q16, int64_t info[8]);
