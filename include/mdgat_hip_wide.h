/* The fp32-class per-op entries for ragged batches in WIDE slots: frames of up to 2048 keypoints, where the entries of mdgat_hip.h hold
 * 512 (MDGAT_RAGGED_FP32_MAX_KEYPOINTS).  Opt-in by calling them: nothing declared in mdgat_hip.h changes its behaviour.  The layout of a
 * ragged batch, the counts and their checks, the status codes and mdgat_last_error are mdgat_hip.h's. */
#ifndef MDGAT_HIP_WIDE_H
#define MDGAT_HIP_WIDE_H

#include "mdgat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS 2048   /* keypoints per frame the entries below take */

/* The slots of the fp32-class ragged plan of a handle: mdgat_forward_ragged, mdgat_forward_frames_ragged on an MDGAT_ARITH_FP32 handle, and the
 * fp64 handle that runs the encoders alone (a float32 'FPFH_gloabal' module).  mode 0 (the default): Np, Mp <= MDGAT_RAGGED_FP32_MAX_KEYPOINTS,
 * today's behaviour and bits.  mode 1 (wide): Np, Mp <= MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS - slots within 512 x 512 run exactly what they run
 * under mode 0, larger ones the kernels of the per-op entries below; the Sinkhorn form follows mdgat_set_ragged_sinkhorn as before (0: one
 * workgroup per pair, 1 and 2: the split form); beyond 2048 the entries refuse with MDGAT_ERR_UNSUPPORTED, naming 2048.  mdgat_workspace_bytes
 * follows the mode: size the workspace AFTER changing it.  Returns the previous mode, or -1 for a null handle or a bad mode. */
int mdgat_set_ragged_fp32_slots(mdgat_handle* h, int mode);

/* The ragged attention entry of mdgat_hip.h, mdgat_attention_ragged, in WIDE slots: Np, Mp <= MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS (else MDGAT_ERR_UNSUPPORTED, naming 2048), the same contract and
 * checks, under this entry's name.  Slots of at most 512 keys run what mdgat_attention_ragged runs, the same bits.  Beyond, again from the slots
 * alone: full attention on the windowed kernel's ragged instantiation (index 3), a dynamic layer on the wide kernels' - four waves per query
 * tile up to 1024 keys per slot (index 9, 16 with sel), eight up to 2048 (10, 17) - with the uniform launch's geometry for the slots; a dynamic
 * layer always takes a dynamic form.  mdgat_attention_launches counts them under those indices, mdgat_ragged_wide_launches apart. */
int mdgat_attention_ragged_wide(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                const int32_t* counts1_host, int cross, int topk, const float* qkv, float* msg, uint32_t* sel,
                                void* workspace, size_t workspace_bytes, void* stream);

/* The two fp32 ragged Sinkhorn entries of mdgat_hip.h - mdgat_sinkhorn_ragged, mdgat_sinkhorn_extract_ragged - in WIDE slots: Np, Mp <= MDGAT_RAGGED_FP32_WIDE_MAX_KEYPOINTS (else MDGAT_ERR_UNSUPPORTED, naming 2048); the same
 * layout, the same checks under the entry's own name, the same fixed outputs beyond the counts.  split = 0: the one-workgroup-per-pair
 * kernel.  A slot within 512 x 512 runs what mdgat_sinkhorn_ragged runs, the same bits; more than 512 (1024) columns select the ragged twins
 * of sinkhorn_kernel<16, 8> (<32, 8>), and pair b's results are again those of the pair run alone through the uniform entry without a
 * workspace, bit for bit.  split != 0: where the slot has two slabs of 128 rows or more, the split form - a pair's rows over
 * ceil(Np / 128) <= 16 workgroups, one launch per iteration and a finishing one, nobody waits for anybody (csrc/sinkhorn.hip) - whose
 * results agree with the one-workgroup kernel's to fp32 rounding (the column sums merge in another order) and depend on the pair's own
 * scores and its slot alone; a slot of one slab keeps the one-workgroup kernel.  bin_score, iters, mode: as above.
 * workspace (256-byte aligned, mdgat_sinkhorn_ragged_wide_workspace_bytes(B, Np, Mp); 0 for a slot beyond 2048): a Z of the slot's size
 * (used by the extraction entry when Z_or_null is NULL) with the split form's scratch behind it.  It is needed - whole - where either is:
 * by mdgat_sinkhorn_ragged_wide under split != 0 in a slot of two slabs or more, by the extraction entry then and whenever Z_or_null is
 * NULL; otherwise it may be NULL.  Nothing in it is read before the call wrote it.
 * mdgat_ragged_wide_launches: the launches that only a wide slot reaches - these entries' and mdgat_attention_ragged_wide's - counts[i] =
 * launches of index i by this process so far (relaxed atomic counters, never reset: read them before and after a call and subtract):
 *    0 sinkhorn_kernel<16, 8, RAGGED>   1 sinkhorn_kernel<32, 8, RAGGED>   (mdgat_sinkhorn_launches does not count these two)
 *    2 an iteration launch of the split form in a slot beyond 512 x 512    3 its finishing launch
 *    4 attention_kernel<false, 8, LARGE, RAGGED> (windowed full attention)
 *    5 attention_topk_wide_kernel<4, RAGGED>   6 the same with the tap   7 attention_topk_wide_kernel<8, RAGGED>   8 the same with the tap
 *      (4 .. 8 are counted by mdgat_attention_launches as well, under the uniform sibling's form)
 * (The split form in a slot within 512 x 512, and extract_kernel, are counted where they were.) */
#define MDGAT_RAGGED_WIDE_COUNTERS 9
size_t mdgat_sinkhorn_ragged_wide_workspace_bytes(int B, int Np, int Mp);
int mdgat_sinkhorn_ragged_wide(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                               const int32_t* counts1_host, const float* scores, float bin_score, int iters, float* Z, int split,
                               void* workspace, size_t workspace_bytes, void* stream);
int mdgat_sinkhorn_extract_ragged_wide(int B, int Np, int Mp, const int32_t* counts0, const int32_t* counts1, const int32_t* counts0_host,
                                       const int32_t* counts1_host, const float* scores, float bin_score, int iters, int mode,
                                       float match_threshold, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                                       float* Z_or_null, int split, void* workspace, size_t workspace_bytes, void* stream);
void mdgat_ragged_wide_launches(uint64_t counts[MDGAT_RAGGED_WIDE_COUNTERS]);

#ifdef __cplusplus
}
#endif

#endif
