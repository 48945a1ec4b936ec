/* Part of the C ABI of libhbird_hip.so: the mean-centred form of the certified fp16 screen's candidate copy.
 * Included by hbird_hip.h (inside its extern "C" block, after hb_index_t and hb_multi_t are declared); not meant to be included on its own.
 *
 * The screen's certificate bounds |fp16 score - exact score| by E ~ ||q|| max ||b|| 2^-10 (hb_index_set_fp16).  On banks whose rows share a
 * large component -- ViT tokens with massive activations: a few dimensions at 30-100 x the rest, the same sign on every row -- that bound is
 * wider than the gap between rank k and rank k', and every query fails its first certificate.  For any vector mu and scalar t
 *     q.b = (q - t mu).(b - mu) + t mu.(b - mu) + q.mu
 * so the candidate pass may run on fp16 images of the CENTRED operands (mu = the bank's column mean when the copy is made, t = the mean of
 * q.mu / mu.mu over the search's queries): the per-row term enters through the pass' row-init values, the per-query term is added back
 * wherever the re-rank compares a pass score with an exact one, and the bound becomes E' ~ ||q - t mu|| max ||b - mu|| 2^-10.
 * The exact re-rank reads the original fp32 rows: results are the fp32 search's, bit for bit, with centring on or off.
 *
 * hb_index_set_fp16_centre(ix, on): 0 on a new index (the plain copy: every search runs the launches it ran before this entry existed).
 *   A change drops an existing fp16 copy, so the next screened search rebuilds it in the new form.  Rows appended after the copy exists
 *   are converted with the same mu; hb_index_reset, or a capacity change that drops the copy, derives mu anew.  A bank whose column mean is
 *   zero or not finite keeps the plain copy.  Memory: two floats per row beside the copy.
 * hb_index_fp16_centre_info(ix, out): out[0] = 1 when the fp16 copy holds centred rows, out[1] = ||mu||, out[2] = max ||b - mu||,
 *   out[3] = max ||b||, out[4] = t of the last centred search, out[5] = rows converted with mu, out[6] = the setting,
 *   out[7] = 1 when the last search of a caller ran its candidate pass on the centred copy.  Synchronises the index's stream.
 * hb_multi_set_fp16_centre(m, on): hb_index_set_fp16_centre on every shard / replica (each shard derives its own mu). */
#ifndef HBIRD_HIP_CENTRE_H
#define HBIRD_HIP_CENTRE_H
int hb_index_set_fp16_centre(hb_index_t* ix, int on);
int hb_index_fp16_centre_info(const hb_index_t* ix, double out[8]);
int hb_multi_set_fp16_centre(hb_multi_t* m, int on);
#endif /* HBIRD_HIP_CENTRE_H */
