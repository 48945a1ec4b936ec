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
 * hb_multi_set_fp16_centre(m, on): hb_index_set_fp16_centre on every shard / replica (each shard derives its own mu).
 *
 * hb_index_last_centre(ix, mu, scalars, g, init16, bank16, cq, qcn, q16, info): a read-out of what the CONVERSION behind the centred pass
 *   left, for tests of that conversion (hb_index_last_screen, hbird_hip_screen.h, is the same for the pass itself: a wrong mu, g, t or init16
 *   shows in no result, a failing certificate is searched again -- and a cmax or norm that is too SMALL makes the certificate unsound).
 *   Host bookkeeping and copies only: it synchronises the index's stream and launches nothing.  All pointers are HOST pointers and each of
 *   the eight arrays may be NULL; a first call with all of them NULL returns the sizes in info.
 *     info  {rows: rows converted with mu; dp16: halves per row of an fp16 tile (D rounded up to 128); n_mu: floats in mu (= dp16);
 *            n: queries of the last centred pass, 0 when the query side is not valid; level: 0 = that pass was the caller's, 1 = the second
 *            pass over its uncertified queries (which overwrites all three query-side arrays), -1 when the query side is not valid;
 *            n_g = 32 ceil(rows / 32);  n_init = 256 ceil(rows / 256);  n_qpad = 256 ceil(n / 256)}
 *   Bank side -- valid while a centred copy is active (out[0] of hb_index_fp16_centre_info) and holds rows:
 *     mu[n_mu]              the column mean the copy was made with, 0 on the padding dimensions [D, n_mu)
 *     scalars[4]            the device scalars as the floats they are: {cmax = max ||fl32(b - mu)|| over every row converted since mu was
 *                           derived, ||mu|| (both rounded up), mu.mu, t of the last search of a caller}
 *     g[n_g]                per row mu.(b - mu), a k-ascending fmaf chain on the fp32 differences (the last tile's padding rows included)
 *     init16[n_init]        the candidate kernel's row init of the last search of a caller: fmaf(t, g, binit), -inf on the padding rows
 *     bank16[n_g * dp16]    the raw fp16 tiles of the converted row tiles, as uint16.  Layout, as centre_bank_kernel writes it:
 *                           t16[row tile rt][8-group gg][row i][8 halves in k order], 2 * dp16 / 16 = dp16 / 8 groups per tile; component
 *                           k of row r sits at ((r / 32 * (dp16 / 8) + k / 8) * 32 + r % 32) * 8 + k % 8
 *   Query side -- of the last centred pass:
 *     cq[n]                 c_q = q.mu, a k-ascending fmaf chain
 *     qcn[n]                ||fl32(q - t mu)||, rounded up
 *     q16[n_qpad * dp16]    the raw centred query tiles, as uint16, in the bank tiles' layout (the padding queries are zero vectors)
 *   Fails (hb_last_error says which) on a NULL handle or a NULL info; when there is no active centred copy (centring off, no screened search
 *   yet, a bank without a usable mean, hb_index_reset since); and, when cq, qcn or q16 is asked for, when the last search of a caller did not
 *   run centred or hb_index_add, hb_index_reset or a capacity change came after it. */
#ifndef HBIRD_HIP_CENTRE_H
#define HBIRD_HIP_CENTRE_H
int hb_index_set_fp16_centre(hb_index_t* ix, int on);
int hb_index_fp16_centre_info(const hb_index_t* ix, double out[8]);
int hb_multi_set_fp16_centre(hb_multi_t* m, int on);
int hb_index_last_centre(hb_index_t* ix, float* mu, float* scalars, float* g, float* init16, uint16_t* bank16, float* cq, float* qcn, uint16_t* q16, int64_t info[8]);
#endif /* HBIRD_HIP_CENTRE_H */
