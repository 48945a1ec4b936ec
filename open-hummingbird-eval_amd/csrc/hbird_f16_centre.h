// The mean-centred form of the fp16 candidate copy (hbird_f16_centre.hip): its state is a part of the copy (hb_centre_state, hbird_mirror.h);
// here what the searches call and what the re-rank kernels take of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "hbird_mirror.h"

struct hb_index;

// per-query constants of one centred pass, for the re-rank: c_q = q.mu, ||q - t mu||, the state's device scalars
struct hb_centre_view { const float* cq; const float* qcn; const float* sc; };

int hb_centre_convert(hb_index* ix, hipStream_t s, int* centred_out);
int hb_centre_queries(hb_index* ix, int64_t nq, int first, _Float16* q16, hb_centre_view* view, hipStream_t s);
int hb_centre_readout(hb_index* ix, float* mu, float* scalars, float* g, float* init16, uint16_t* bank16, float* cq, float* qcn, uint16_t* q16, int64_t info[8]);
