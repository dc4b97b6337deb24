/*
 * pfhip.h — C ABI of libpfhip.so: the MI355X (gfx950) device path of the background
 * forecasting hot path of nianticlabs/panoptic-forecasting.
 *
 * The reference has no FFI of its own for this path: its "native boundary" is
 * torch.ops.torch_scatter.scatter_min + ATen/cuDNN, reached from
 *   PCTransformModel.predict  panoptic_forecasting/models/pc_transform/pc_transform_model.py:26-150
 *   BGModel.predict           panoptic_forecasting/models/bg/bg_model.py:91-102
 *   hardnet.forward           panoptic_forecasting/models/bg/hardnet.py:353-387
 * Each entry point below names the reference lines it replaces.  The Python
 * shims that bind them (ctypes) are panoptic-forecasting_amd/{lib,pc_transform_model,bg_model}.py;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - every buffer is a caller-owned DEVICE pointer (tensor.data_ptr()); C-contiguous;
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *  - calls only enqueue work on `stream`: no allocation, no host sync, no hidden copies
 *    (plan create/destroy excepted) — they may be captured into a hipGraph;
 *  - every function returns 0 on success or a negative PF_E* code; pf_last_error() gives
 *    the thread-local message;
 *  - one in-flight call per (workspace, stream); plans are immutable after creation and
 *    may be shared between threads/streams.
 */
#ifndef PFHIP_H
#define PFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_OK 0
#define PF_EINVAL (-1)    /* bad argument */
#define PF_EWORKSPACE (-2) /* workspace too small */
#define PF_EBLOB (-3)     /* malformed weight blob */
#define PF_EHIP (-4)      /* HIP runtime error (launch, alloc in plan create) */
#define PF_EUNSUPPORTED (-5)

typedef struct pf_plan pf_plan;

/* ABI version (major*1000 + minor). */
int pf_version(void);
/* Thread-local description of the last failure on this thread ("" if none). */
const char *pf_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Warp + z-buffered splat  — replaces pc_transform_model.py:41-150 (unproject :41-59, cam->vehicle
 * :63, ego warp :68, vehicle->cam + project :71-78, validity :83-89, sentinel :105, 4-corner
 * bins :106-117, torch_scatter.scatter_min :118-119, winner gather :120-139).
 *
 *   depth      [B,T_total,H,W] f32        depth_mask [B,T_total,H,W] u8 (0/1)
 *   seg        [B,T_total,H,W,C] u8       C = seg_channels (1, or 3 for is_img)
 *   Kinv,K     [B,3,3] f32   E,Einv [B,4,4] f32   T_tgt [B,T_total,4,4] f32
 *     (Kinv/Einv are the caller's torch.inverse(K)/torch.inverse(E): LAPACK bits decide floor())
 *   frames t_first .. t_first+T-1 are warped (only_this_ind => t_first=ind, T=1; else 0, T_total).
 *   per_frame is a bit set (PF_SPLAT_*):
 *   PF_SPLAT_PER_FRAME clear: all T frames share ONE z-buffer (reference semantics of a single predict call)
 *                  out_seg [B,H,W,C] u8, out_depth [B,H,W] f32
 *   PF_SPLAT_PER_FRAME set:   every frame gets its own z-buffer and its own sentinel, i.e. T independent
 *                  only_this_ind=t calls in one launch: out_seg [B,T,H,W,C], out_depth [B,T,H,W]
 *   PF_SPLAT_PER_SAMPLE_SENTINEL set: the sentinel max+1 (:105) is taken per sample instead of over the whole batch
 *                  of the call (the reference's `.max()` spans the batch, so the depth written at holes won by
 *                  invalid points depends on which samples share a predict call; with this bit a sample's output is
 *                  what the reference gives for it at batch size 1 — SURVEY.md 8e opt-in)
 *   out_result2d (nullable) [B,T,H,W,2] i64: clamped (x,y) of the floor/floor corner (:147)
 *
 * Winner rule: minimum depth; ties -> lowest source element index e = r*P + t*N + n (r = corner
 * replica 0..3, P = T*N), which is pytorch_scatter's CPU rule.  Bins reached only by invalid
 * points yield seg=0, depth=max+1 (:105,:133); untouched bins seg=0, depth=-1 (:136-138).
 * Out of contract: non-finite projected coordinates, |z| >= 2^24.
 */
#define PF_SPLAT_PER_FRAME 1
#define PF_SPLAT_PER_SAMPLE_SENTINEL 2
int pf_warp_splat_workspace(int B, int T, int H, int W, int per_frame, size_t *bytes);
int pf_warp_splat(const float *depth, const uint8_t *depth_mask, const uint8_t *seg, int seg_channels,
                  const float *Kinv, const float *E, const float *T_tgt, const float *Einv,
                  const float *K, int B, int T_total, int t_first, int T, int H, int W, int per_frame,
                  uint8_t *out_seg, float *out_depth, int64_t *out_result2d,
                  void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * FC-HarDNet-70 bg network — replaces bg_model.py:53-71,91-102 and hardnet.py:353-387.
 *
 * The plan is built from a weight blob (layout: panoptic-forecasting_amd/packing.py — op table +
 * BN-folded fp32 OIHW weights).  Plan creation uploads/re-tiles the weights (allocates device
 * memory once); forward calls allocate nothing.
 */
int pf_hardnet_plan_create(const void *blob_host, size_t bytes, int in_ch, int n_cls, pf_plan **out);
void pf_hardnet_plan_destroy(pf_plan *plan);
int pf_hardnet_workspace(const pf_plan *plan, int B, int H, int W, size_t *bytes);

/* Status of a forward.  The first PF_WS_STATUS_BYTES of a forward's workspace are its status block.  Word 0 is the status
 * word of the LAST FINISHED forward: written once, by the launch that ends a forward (its kernels collect their flags in a
 * private word of the block), so it is final once the stream has run the forward and stays readable while the next one runs.
 * Word 1 (PF_WS_STICKY_OFFSET) is STICKY: every forward ORs its final status word into it and only the host clears it
 * (pf_hardnet_status_sticky(clear = 1), pf_hardnet_status_reset) - the word to read after a hipGraph replay or an eager loop
 * that ran several forwards through one workspace.  The caller ZEROES THE BLOCK ONCE after allocating the workspace
 * (pf_hardnet_status_reset, or a memset): forwards do not start with a memset, the ending launch leaves the block ready for
 * the next one.
 *   PF_STATUS_RANGE      a tensor that feeds the two-term fp16 operand path (option "split_f16") held a value with
 *                        |x| > 65504 (inf included; NaN in a caller-provided input or produced by the stem): fp16 pairs cannot
 *                        represent it, so the outputs of THIS forward are not to be used.
 *   PF_STATUS_RANGE_LOW  the largest |x| a launch stored into such a tensor was non-zero and below 2^-6: the pair keeps an
 *                        absolute 2^-25 below |x| = 0.25, so a tensor of tiny values would lose relative precision that fp32
 *                        keeps.  (Unflagged: every operand within 2^-23 |x| + 2^-25 and 2^-25 <= 2^-19 of the tensor's maximum.)
 *                        Plan creation already stores every channel multiplied by a power of two that puts its expected
 *                        magnitude at 8 (an exact re-parameterisation of the folded weights, option "normalize_ranges"), so this
 *                        fires only for data far from what the weights suggest.
 * Either bit: the reference's fp32 Conv2d (hardnet.py:16-25) has no such limits - re-run the forward with plan option
 * "split_f16" = 0 (what BGModel does by default, bg_model.py `on_range_overflow`) or fail.  Never raised by fp32-only plans.
 * A caller that manages streams itself reads the words with its outputs (ordinary device memory; BGModel copies them to pinned
 * host memory behind every forward and checks them lazily); pf_hardnet_status / pf_hardnet_status_sticky are the convenience
 * forms: they copy a word to the host and SYNCHRONISE `stream` (the only calls of this library that wait for the device).
 * pf_hardnet_range_maxima: max |stored value| per op of the plan's table in the last forward (0 for ops that keep none), a
 * diagnostic for the guard (synchronises). */
#define PF_STATUS_RANGE 1u
#define PF_STATUS_RANGE_LOW 2u
#define PF_WS_STATUS_OFFSET 0
#define PF_WS_STICKY_OFFSET 4
#define PF_WS_STATUS_BYTES 2048
int pf_hardnet_status(const void *ws, unsigned *status, void *stream);
int pf_hardnet_status_sticky(void *ws, unsigned *status, int clear, void *stream);
int pf_hardnet_status_reset(void *ws, void *stream);
int pf_hardnet_range_maxima(const pf_plan *plan, const void *ws, float *maxima, int cap, int *n_ops, void *stream);

/* hop_flags: emulate the reference's on-disk hop between the two tasks on the fly */
#define PF_HOP_NONE 0
#define PF_HOP_TRAINID_LUT 1 /* seg ids -> trainIds (export_cityscapes_segmentation_results.py:34-38) */
#define PF_HOP_DEPTH_U16 2   /* depth -> round(clamp(d+1,0,255)*256) u16 (:119-124) -> x/256-1, mask=d>0,
                                d[~mask]=-1, clamp to [min_depth,max_depth] (bg_dataset.py:224-230,166-170);
                                depth_mask argument is ignored (may be NULL) */

/*
 * Fused forward: one-hot of T label maps (labels >= n_cls -> zero vector, bg_model.py:53-59) +
 * normalised masked depth (:50-51,:66-68) feed the stem conv directly (the [B,36,H,W] tensor is never
 * materialised), then hardnet (hardnet.py:353-371), bilinear align_corners upsample to (out_h,out_w)
 * (:372-384) and argmax (bg_model.py:98).
 *   seg   [B,T,H,W] u8 or i64 (seg_is_i64)      depth [B,T,H,W] f32     depth_mask [B,T,H,W] u8
 *   out_seg [B,out_h,out_w] u8 or i64 (out_seg_is_i64)
 *   out_logits (nullable) [B,n_cls,out_h,out_w] f32; out_orig_logits (nullable) [B,n_cls,H/4,W/4] f32
 */
int pf_bg_forward(const pf_plan *plan, const void *seg, int seg_is_i64, const float *depth,
                  const uint8_t *depth_mask, float depth_mean, float depth_std, int hop_flags,
                  float min_depth, float max_depth, int B, int T, int H, int W, int out_h, int out_w,
                  void *out_seg, int out_seg_is_i64, float *out_logits, float *out_orig_logits,
                  void *ws, size_t ws_bytes, void *stream);

/* Dense-input forward (convert2onehot=False configurations, bg_model.py:61-71): x [B,in_ch,H,W] f32. */
int pf_hardnet_forward_dense(const pf_plan *plan, const float *x, int B, int H, int W, int out_h,
                             int out_w, void *out_seg, int out_seg_is_i64, float *out_logits,
                             float *out_orig_logits, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * The on-disk hop between the reference's tasks, device side.  Elementwise, HBM-bound.
 *
 * pf_hop_export — what export_results applies to a prediction before the PNG encoder
 * (experiments/export_cityscapes_segmentation_results.py):
 *   seg [n] u8 or i64 (nullable) -> out_seg [n] u8; seg_mode 0 = as is (--no_convert), 1 = trainId -> label id
 *   (convert_labels :27-32, values outside 0..18 -> 0), 2 = label id -> trainId (convert_labels_to_trainid :34-38,
 *   ids outside the table -> 0);  depth [n] f32 (nullable) -> out_depth_u16 [n] = round(clamp(d+1,0,255)*256) (:119-121).
 * pf_hop_load — what BGDataset.__getitem__ applies to the u16 depth it reads (data/datasets/bg_dataset.py:224-228,
 *   166-170): d = q/256 - 1, mask = d > 0, d[~mask] = -1, masked values clamped to [min_depth, max_depth].
 * All buffers 16-byte aligned device pointers.
 */
int pf_hop_export(const void *seg, int seg_is_i64, int seg_mode, const float *depth, size_t n, uint8_t *out_seg,
                  uint16_t *out_depth_u16, void *stream);
int pf_hop_load(const uint16_t *depth_u16, size_t n, float min_depth, float max_depth, float *out_depth,
                uint8_t *out_mask, void *stream);

/* ------------------------------------------------------------------------------------------
 * Training-time augmentation of BGDataset (data/transforms.py:183-293: joint random scale / pad / crop / nearest resize /
 * flip) fused with the depth decode of the load hop - ONE launch per batch, enqueue only, no workspace.  Every step of the
 * transform acts on one axis, so a sample's transform is four index tables built on the host (bg_augment.py):
 *     out[y][x] = src[y_tab[y]][x_tab[x]],   entry j = source row / column of output row / column j.
 *
 *   seg_src   [B,T,Hs,Ws] u8        label_src [B,Hs,Ws] u8 or NULL       depth_src [B,T,Hs,Ws] u16 codes or NULL
 *   y_map [B,oh], x_map [B,ow] i32  tables of the label maps (seg_src, label_src)
 *   y_arr [B,oh], x_arr [B,ow] i32  tables of the depth arrays (may be NULL when depth_src is NULL)
 *   out_seg [B,T,oh,ow] u8, out_label [B,oh,ow] u8, out_depth [B,T,oh,ow] f32, out_mask [B,T,oh,ow] u8 (0/1): the layout
 *   pf_train_forward_backward takes (seg_is_i64 = 0, labels_are_i64 = 0); outputs of a NULL input are not written.
 *
 * A table entry outside [0,Hs) resp. [0,Ws) is padding and is never followed as an address: padding gives pad_label (0..255)
 * in seg and label, and depth code 0, which decodes to -1 with mask 0.  Depth codes decode exactly as in pf_hop_load.
 * With ow % 4 == 0, out_depth 16-byte and the u8 outputs 4-byte aligned the stores are 16 / 4 bytes per lane; any other
 * width or alignment (out_depth at least 4-byte, depth_src 2-byte, tables 4-byte) takes scalar stores.  ow <= 8192 (the x
 * tables are staged in LDS), else PF_EUNSUPPORTED.  B = 0 launches nothing.
 */
int pf_bg_augment(const uint8_t *seg_src, const uint8_t *label_src, const uint16_t *depth_src, int B, int T, int Hs, int Ws,
                  const int *y_map, const int *x_map, const int *y_arr, const int *x_arr, int oh, int ow, int pad_label,
                  float min_depth, float max_depth, uint8_t *out_seg, uint8_t *out_label, float *out_depth,
                  uint8_t *out_mask, void *stream);

/* ------------------------------------------------------------------------------------------
 * Batch assembly of the fg export path — what FGSceneDataset.__getitem__ (data/datasets/fg_scene_dataset.py:380-454)
 * computes per scene after the has_gt rows and bbox_inds columns are selected, for all N instances of a batch in ONE launch:
 * enqueue only, no workspace, a single kernel node.  N = 0 launches nothing.  T = 6 (else PF_EUNSUPPORTED), 0 <= T_in <= T.
 *
 *   bboxes [N,T,4] f32 ulbr as stored       feat_mask [N,T] u8       depth [N,T] f32       classes [N] i32 trainIds
 *   feat_row [N,T_in] i32 row of feat_table or -1      feat_table [M,256,14,14] f32 (NULL when M = 0)
 *   use_ulbr: keep ulbr, else convert_bbox_ulbr_cwh;  max_depth < 0: no depth bound;  filter_car_gap < 0: no car-gap filter
 *   (_filter_car_gap :300-340 for class 13: it reads x0 / x1 from the boxes AFTER the conversion - restated, not repaired);
 *   img_w: the image width the filter measures from (2048).  The two doubles are rounded to fp32 once, as torch rounds a
 *   Python number it compares with a float32 tensor; img_w - filter_car_gap is formed in double and rounded once.
 *
 *   trajectories [N,T,8] (box, velocity)   bbox_masks, bbox_vel_masks, feat_masks, depth_masks [N,T] u8 (0/1)
 *   depths [N,T,2] (depth, velocity)       classes_out [N] i64 = class - 11        one_hot_classes [N,8] f32
 *   final_bboxes [N,4] = the last step's box      feats [N,T_in,256,14,14] = the gathered plane, or zeros
 *
 * Every step is one fp32 operation in the reference's order: all outputs are bit-identical to torch's.  A feat_row outside
 * [0,M) is never followed as an address: its plane is zeros.  bboxes, feat_table, trajectories, one_hot_classes,
 * final_bboxes and feats must be 16-byte aligned (the gather moves 16 bytes per lane and access).
 */
int pf_fg_assemble(const float *bboxes, const uint8_t *feat_mask, const float *depth, const int32_t *classes,
                   const int32_t *feat_row, const float *feat_table, int N, int T, int T_in, int M, int use_ulbr,
                   double max_depth, double filter_car_gap, int img_w, float *trajectories, uint8_t *bbox_masks,
                   uint8_t *bbox_vel_masks, uint8_t *feat_masks, float *depths, uint8_t *depth_masks, int64_t *classes_out,
                   float *one_hot_classes, float *final_bboxes, float *feats, void *stream);

/* ------------------------------------------------------------------------------------------
 * fg -> panoptic merge — replaces the pasting loops of FGModel.predict_panoptic
 * (models/fg/fg_model.py:548-588; panoptic_ids=1, clear_things=1) and FGModel.predict_semantics (:455-480; panoptic_ids=0,
 * clear_things=0) together with model_utils.paste_mask (models/fg/model_utils.py:30-57).
 *
 *   background    [B,H,W] u8 / i32 / i64 (bg_kind 0/1/2) trainId canvas, or NULL (canvas of 255, :517-518)
 *   bg_depth      [B,H,W] f32 or NULL;  bg_depth_mask [B,H,W] u8 or NULL (0 -> depth 1e9, :563-564)
 *   masks         [N,MH,MW] f32 mask PROBABILITIES (after the sigmoid of :532), all images concatenated
 *   boxes         [N,4] f32 (cx,cy,w,h), or (x0,y0,x1,y1) when box_is_ulbr
 *   inst_depth    [N] f32 forecast depth per instance (required with use_depth_sorting)
 *   classes       [N] i64 thing class (0..7);  inst_offsets [B+1] i32: image b owns instances [off[b], off[b+1])
 *   out           [B,H,W] i32 or i64
 * Paste order: descending depth, stable (ATen's CPU sort) when use_depth_sorting, else index order.  A pixel takes
 * an instance's value where its bilinearly pasted mask is >= 0.5 and - when bg_depth is given - its depth is strictly
 * nearer than the current one (:580-585); value = (class+11)*1000 + running per-class id (:568-572) or class+11.
 * The mask sampling reproduces F.grid_sample(bilinear, zeros, align_corners=False) of ATen's vectorised CPU kernel
 * bit for bit.  Unlike the reference, the caller's bg_depth tensor is not modified.  W % 4 == 0.
 * Workspace: pf_panoptic_merge_workspace(n_instances) bytes.
 *
 * pf_panoptic_encode — export_cityscapes_panoptic_results.py:27-68: ids converted to Cityscapes ids when
 * convert_to_ids (255 -> 0; v > 100: id(cat)*1000 + inst; else id(v)), out_rgb [B,H,W,3] = (id%256, id/256%256,
 * id/65536), out_ids (nullable) [B,H,W] i32, out_present [B, pf_panoptic_max_ids()] u8 = 1 for every id that occurs
 * (get_segments_info's np.unique).  H*W % 4 == 0.
 */
int pf_panoptic_merge_workspace(int n_instances, size_t *bytes);
int pf_panoptic_merge(const void *background, int bg_kind, const float *bg_depth, const uint8_t *bg_depth_mask,
                      const float *masks, int MH, int MW, const float *boxes, int box_is_ulbr,
                      const float *inst_depth, const int64_t *classes, const int32_t *inst_offsets,
                      int n_instances, int B, int H, int W, int use_depth_sorting, int panoptic_ids,
                      int clear_things, void *out, int out_is_i64, void *ws, size_t ws_bytes, void *stream);
int pf_panoptic_encode(const void *seg, int seg_is_i64, int convert_to_ids, int B, int H, int W, uint8_t *out_rgb,
                       int32_t *out_ids, uint8_t *out_present, void *stream);
int pf_panoptic_max_ids(void);

/* ------------------------------------------------------------------------------------------
 * Panoptic quality — the segment matching of the evaluation that ends scripts/fg/run_fg_eval_panoptic.sh
 * (cityscapesscripts.evaluation.evalPanopticSemanticLabeling; absent and unpinned here: layout and parity unpinned).
 *
 *   pred, gt    [B,H,W] i32 or i64 label maps, each width chosen on its own; both are only read.  H*W % 4 == 0, 16-byte aligned.
 *   fmt 0       trainId format (the merge output): stuff = trainId, thing = trainId*1000 + instance, void = 255;
 *               category = v/1000 for v >= 1000, else v.
 *   fmt 1       Cityscapes id format (what the exported / ground-truth PNG decodes to): void = 0; category id = v/1000 for
 *               v >= 1000, else v, mapped to its trainId by the inverse of the export's trainId -> id table.
 *   A pixel is VOID when its category is none of the n_cls (<= 19) evaluated classes; void is one pseudo-segment, every other
 *   segment is identified by its raw value.  With crowd != 0 a ground-truth segment is CROWD iff it has no instance part
 *   (v < 1000) and its trainId is a thing class (11..18), as the Cityscapes panoptic ground truth marks iscrowd.
 *   TP   gt segment neither void nor crowd, same category as the prediction, and
 *        iou = inter / (g_area + p_area - inter - p_void[p]) > 0.5 strictly (p_void[p]: pixels of p on void ground truth).
 *   FN   a gt segment, neither void nor crowd, without a match.
 *   FP   a non-void predicted segment without a match, unless p_void + p_crowd > 0.5 * p_area strictly, p_crowd being its
 *        pixels on crowd ground truth of its own category.  A crowd segment is never TP or FN; its pixels stay in the union.
 *   acc         [n_cls,4] f64 (sum_iou, TP, FP, FN), ADDED to; per_image (nullable) [B,n_cls,4] f64, written.
 * Areas and counts are integers, an iou is one fp64 division; the ious of a class are added in ascending gt id inside an
 * image and the images in index order, so two runs of a call give the same bits although the tables are filled by integer
 * atomics.  Tables: pf_pq_table_slots() = 8192 distinct (gt, pred) pairs per image (a Cityscapes image has a few hundred);
 * 1024-slot tables in LDS in front of them, whose overflow spills to the image's table without loss.
 * Never silent: the first word of the workspace is a sticky status word, ORed with
 *   PF_PQ_STATUS_FULL   an image had more distinct pairs than pf_pq_table_slots()
 *   PF_PQ_STATUS_VALUE  a value outside [0, 65536) (compared in the map's own width: 2^33 + 5 is out of range)
 * and an image flagged with either adds nothing to acc (its per_image row is zero).  The caller zeroes the first 256
 * bytes of a fresh workspace once (pf_pq_status_reset enqueues that); everything else is zeroed by every call with the
 * library's own fill kernel, so a captured call holds kernel nodes only.  pf_pq_accumulate enqueues only (4 launches);
 * B == 0 launches nothing.  pf_pq_status copies the status word to the host and waits for the stream.
 */
#define PF_PQ_STATUS_FULL 1u
#define PF_PQ_STATUS_VALUE 2u
int pf_pq_workspace(int B, size_t *bytes);
int pf_pq_table_slots(void);
int pf_pq_accumulate(const void *pred, int pred_is_i64, const void *gt, int gt_is_i64, int fmt, int crowd, int n_cls, int B,
                     int H, int W, double *acc, double *per_image, void *ws, size_t ws_bytes, void *stream);
int pf_pq_status(const void *ws, void *stream, int *host_status);
int pf_pq_status_reset(void *ws, void *stream);

/* ------------------------------------------------------------------------------------------
 * Semantic confusion matrix — the pixel counts behind IoU / mIoU of the Cityscapes pixel-level evaluation
 * (cityscapesscripts.evaluation.evalPixelLevelSemanticLabeling; absent and unpinned here: parity unpinned).
 *
 *   pred, gt    [B,H,W] label maps, each of its own kind: 0 = u8, 1 = i32, 2 = i64; both are only read.  u8 is the native case
 *               (exported PNGs and the model's own maps are bytes).  A base pointer need only be aligned to its element: heads and
 *               tails of an image that do not fill a 16-byte load are read per element.
 *   fmt 0       trainId format: values 0..18 are classes, everything else (255 included) is void.
 *   fmt 1       Cityscapes labelIds, mapped through the inverse of the export's trainId -> id table; every id without a trainId is void.
 *   A value whose class is >= n_cls (1..19) is void.
 *   acc         [20,20] i64, ADDED to: row = ground-truth class, column = predicted class, index 19 = void.
 *   per_image   (nullable) [B,20,20] i64, written.
 * Integers only - there is no floating-point operation on the device - so two runs of a call give the same bits.  A workgroup of
 * the count pass owns pf_confusion_chunk_pixels() = 16384 pixels of one image.
 * Never silent: the first word of the workspace is a sticky status word, ORed with
 *   PF_CONF_STATUS_VALUE  a value outside [0, 256) in an i32 / i64 map (compared in the map's own width: 2^33 + 5 is out of range)
 * and an image flagged with it adds nothing to acc (its per_image block is zero).  The caller zeroes the first 256 bytes of a fresh
 * workspace once (pf_confusion_status_reset enqueues that); everything else is zeroed by every call with the library's own fill
 * kernel, so a captured call holds kernel nodes only.  pf_confusion_accumulate enqueues only (3 launches); B == 0 launches nothing.
 * pf_confusion_status copies the status word to the host and waits for the stream.
 */
#define PF_CONF_STATUS_VALUE 1u
int pf_confusion_workspace(int B, size_t *bytes);
int pf_confusion_chunk_pixels(void);
int pf_confusion_accumulate(const void *pred, int pred_kind, const void *gt, int gt_kind, int fmt, int n_cls, int B, int H, int W,
                            long long *acc, long long *per_image, void *ws, size_t ws_bytes, void *stream);
int pf_confusion_status(const void *ws, void *stream, int *host_status);
int pf_confusion_status_reset(void *ws, void *stream);

/* ------------------------------------------------------------------------------------------
 * Instance-weighted IoU (iIoU) — the per-instance sums behind "classes iIoU" / "categories iIoU" of the same evaluator (written
 * down as remembered: parity unpinned).  Called beside pf_confusion_accumulate on the same predictions; the false positives of
 * the score come from that call's [20,20] table.
 *
 *   pred        [B,H,W] prediction label map in fmt: 0 = u8, 1 = i32, 2 = i64 (as above).
 *   inst        [B,H,W] ground-truth instance map (*_gtFine_instanceIds.png): 0 = u16, 1 = i32, 2 = i64; ALWAYS Cityscapes labelIds,
 *               whatever fmt says about the prediction.  A value v > 1000 is the instance labelId * 1000 + k of its image (label
 *               v / 1000, index k = v % 1000); it counts when its label's trainId c has 11 <= c < n_cls (person 24 .. bicycle 33).
 *               Every other value is ignored without an error (v <= 1000, caravan 29xxx, trailer 30xxx, labels without a trainId).
 *               Base pointers need only be aligned to their element, as above.
 *   fmt 0 / 1   a pixel of an instance is a true positive when its prediction equals c (trainId format) / the labelId (Cityscapes).
 *   Per instance of `size` pixels, `tp` of them true positives, in float64, each operation rounded once, never fused:
 *               w = avg[c] / size;  tpw = tp * w;  fnw = (size - tp) * w        (avg: the evaluator's class-size table)
 *   Per image and class the terms are added in ascending v, from 0.0, into (itp, ifn): an image's pairs are bit-identical
 *   whatever batch it is in.
 *   acc_inst          [8][2] f64 (itp, ifn) per thing class 11..18, ADDED to, image by image in batch order.
 *   acc_counts        [8][3] i64 (instances, their pixels, their true-positive pixels), ADDED to.
 *   per_image         (nullable) [B][8][2] f64, written.      per_image_counts  (nullable) [B][8][3] i64, written.
 * The count pass is integers only (an image's u32 [8][1000][2] table of (size, tp) in the workspace, filled with integer atomics:
 * the order they arrive in does not matter); a workgroup of it owns pf_iiou_chunk_pixels() = 16384 pixels of one image.  The
 * first word of the workspace is a sticky status word of its own, ORed with
 *   PF_IIOU_STATUS_VALUE  a prediction value outside [0, 256) or an instance value outside [0, 65536) in an i32 / i64 map (compared
 *                         in the map's own width: 2^33 + 5 is out of range)
 * and an image flagged with it adds nothing (its per-image blocks are zero).  The caller zeroes the first 256 bytes of a fresh
 * workspace once (pf_iiou_status_reset enqueues that); everything else is zeroed by every call with the library's own fill
 * kernel, so a captured call holds kernel nodes only.  pf_iiou_accumulate enqueues only (4 launches: fill, count, weigh, finish);
 * B == 0 launches nothing.  pf_iiou_status copies the status word to the host and waits for the stream.
 */
#define PF_IIOU_STATUS_VALUE 1u
int pf_iiou_workspace(int B, size_t *bytes);
int pf_iiou_chunk_pixels(void);
int pf_iiou_accumulate(const void *pred, int pred_kind, const void *inst, int inst_kind, int fmt, int n_cls, int B, int H, int W,
                       double *acc_inst, long long *acc_counts, double *per_image, long long *per_image_counts, void *ws,
                       size_t ws_bytes, void *stream);
int pf_iiou_status(const void *ws, void *stream, int *host_status);
int pf_iiou_status_reset(void *ws, void *stream);

/* ------------------------------------------------------------------------------------------
 * Instance AP — the integer records behind AP / AP50 of the Cityscapes instance-level evaluation
 * (cityscapesscripts.evaluation.evalInstanceLevelSemanticLabeling: absent here; the definition below is written down from that
 * evaluator as remembered: parity unpinned).  pf_ap_accumulate intersects every predicted mask with every ground-truth region of
 * its label; everything after the records is float64 on the host (instance_ap.ap_from_records).
 *
 * Constants.  Instance classes are labelIds 24, 25, 26, 27, 28, 31, 32, 33 (person .. bicycle; trainIds 11..18), in that order
 *   class index 0..7.  The overlap thresholds are the float64 values of np.arange(0.5, 1.0, 0.05), taken verbatim and not as
 *   rounded decimals: the third is 0.6000000000000001.  min_region is an integer parameter, default 100.  The distance criteria
 *   of the original (AP50m / AP100m) are not built.
 * Ground truth.  In an image's instance map a value v < 1000 is the labelId v with no instance; for an instance class this is a
 *   *group*.  A value v >= 1000 is instance v % 1000 of label v / 1000.  Void pixels are those whose value is the id of an
 *   ignore_in_eval label (csrc/gt_labels.h).  A ground-truth region of class c is *regular* when v >= 1000 and its pixel count
 *   is >= min_region.
 * Prediction p.  A binary mask (inside = non-zero), a labelId and a confidence.  It is *skipped* if its label is not an instance
 *   class or its mask is empty; otherwise it is *counted*.
 * Per counted prediction, integers only.  `pixels` is the mask's pixel count.  For every ground-truth value g of the same label
 *   (regular, small or group) inter(p, g) is the intersection pixel count.
 *   ignore = |mask & void| + sum of inter(p, g) over groups + sum of inter(p, g) over g with fewer than min_region pixels; a
 *   small group is added twice, as in the original.  `best` is the g with the largest non-zero intersection, ties to the smaller
 *   value; its value, inter and g's own pixel count are recorded.  Only `best` matters at every threshold: an overlap
 *   inter / (|g| + pixels - inter) > 0.5 forces inter > pixels / 2, so the full pairwise matching of the original reduces to it.
 * Per class c and threshold t, over all images.  A counted prediction *hits* when its best exists and
 *   float(inter) / (|g| + pixels - inter) > t.  A hit on a regular g: among the predictions of that image hitting that g the one
 *   of highest confidence is a true positive (1, conf), the others are false positives (0, conf); equal confidences are
 *   indistinguishable in the lists.  A hit on a group or a small region: the prediction is dropped.  No hit: it is a false
 *   positive (0, conf) when float(ignore) / pixels <= t, else it is dropped.  hard_fn is the number of regular g that no
 *   prediction hits.
 * AP.  have_gt: any image has a regular g of c.  have_pred: any image has a counted prediction of c.  AP is nan without have_gt
 *   and 0.0 with have_gt but without have_pred.  AP is 0.0 when every prediction was dropped (the original would raise there).
 *   Otherwise the original's curve: sort the scores ascending; take the unique scores with their first indices; for each
 *   tp = n_true - cum[idx - 1], fp = n - idx - tp, fn = cum[idx - 1] + hard_fn (0 appended to the cumulative sum, so index -1
 *   reads 0); append precision 1 and recall 0; the step widths are np.convolve([r0, r..., 0], [-0.5, 0, 0.5], 'valid'); AP is
 *   precision . widths.  The result does not depend on the order of the records.  Reported: per class `ap` (mean over the ten
 *   thresholds) and `ap50%`; allAp, the nan-mean over classes x thresholds; allAp50%, the nan-mean over classes at t = 0.5.
 *
 *   masks       [P][H][W] u8, inside = non-zero; any base alignment.
 *   mask_image  [P] i32, the index of the mask's image in gt; may be unsorted, an image's masks need not be contiguous.
 *   mask_label  [P] i32, a labelId.
 *   gt          [B][H][W] instance map (*_gtFine_instanceIds.png): gt_kind 0 = u16, 1 = i32, 2 = i64, aligned to its element.
 *   rec         [P][8] i32, written: {state, pixels, ignore, best_value (-1: none), best_inter, best_pixels, image, class index}.
 *               state 0 counted, 1 empty, 2 not an instance class, 3 flagged.  Only a counted record carries counts (the others
 *               hold pixels = ignore = best_inter = best_pixels = 0 and best_value = -1); image is mask_image as given; class
 *               index is -1 where the label is no instance class or out of range.
 *   gt_regular  [B][8] i32, written: the number of regular regions per class; zero for a flagged image.
 * Passes (5 launches: fill, size, overlap, record, regular; all kernel nodes): the size pass scans gt alone into a dense per-image
 * table u32 [8][1008] of region sizes (1000 instances + the group per class); the overlap pass (grid: chunks of
 * pf_ap_chunk_pixels() = 16384 pixels x P) folds runs of equal (inside, value) in registers, classifies a run inside the mask once
 * and counts it in a dense 4 KB table in LDS (1000 instances + group + void + pixels of the prediction's own label), added to the
 * prediction's u32 [1024] table in the workspace with integer atomics; one wave per prediction then writes rec, one workgroup per
 * image gt_regular.  No floating point on the device.  P == 0 runs the fill, size and regular passes only, B == 0 the record pass
 * only (every prediction is flagged; nothing of the workspace but the status word is touched).  H * W must be below 2^30, P and B at most 65535.
 * The first word of the workspace is a sticky status word of its own, ORed with
 *   PF_AP_STATUS_VALUE  a gt value outside [0, 65536), compared in the map's own width.  The image and its predictions are
 *                       flagged and add nothing.
 *   PF_AP_STATUS_INDEX  a mask_image outside [0, B) or a mask_label outside [0, 34).  The prediction is flagged.
 * The caller zeroes the first 256 bytes of a fresh workspace once (pf_ap_status_reset enqueues that); everything else is zeroed by
 * every call with the library's own fill kernel.  pf_ap_status copies the status word to the host and waits for the stream.
 */
#define PF_AP_STATUS_VALUE 1u
#define PF_AP_STATUS_INDEX 2u
int pf_ap_workspace(int P, int B, size_t *bytes);
int pf_ap_chunk_pixels(void);
int pf_ap_accumulate(const void *masks, const int *mask_image, const int *mask_label, int P, const void *gt, int gt_kind, int B, int H,
                     int W, int min_region, int *rec, int *gt_regular, void *ws, size_t ws_bytes, void *stream);
int pf_ap_status(const void *ws, void *stream, int *host_status);
int pf_ap_status_reset(void *ws, void *stream);
/* Host only, nothing enqueued (tests): the slot of the overlap pass's table that a pixel inside a mask of `label` adds to when the
 * ground truth holds `value`: 0..999 instance k, 1000 the group, 1001 void, -1 neither (or label is no instance class). */
int pf_debug_ap_slot(int value, int label, int *slot);

/* ------------------------------------------------------------------------------------------
 * Cityscapes ground-truth preparation — what createPanopticImgs and createTrainIdLabelImgs of cityscapesscripts.preparation (absent
 * here, written down as remembered: parity unpinned) and the reference's scripts/preprocessing/remove_fg_from_gt.py compute, from
 * the one file per image they all derive from.
 *
 *   inst            [B,H,W] instance maps (*_gtFine_instanceIds.png): 0 = u16, 1 = i32, 2 = i64.  A value v below 1000 is a labelId L,
 *                   any other is L * 1000 + instance index.  The base pointer need only be aligned to its element; where the map is
 *                   not 16-byte aligned relative to the outputs it is read per element.
 *   out_rgb         (nullable) [B,H,W,3] u8, the panoptic PNG's pixels: (0,0,0) where L is ignoreInEval, else
 *                   (v % 256, v / 256 % 256, v / 65536).
 *   out_train       (nullable) [B,H,W] u8, the trainId of L; 255 for a label without one.
 *   out_train_nofg  (nullable) [B,H,W] u8, the same with the thing classes (trainIds 11..18: hasInstances and not ignoreInEval)
 *                   replaced by 255.
 *   seg_count       (nullable, with segs) [B] i32;  segs [B][pf_gt_prepare_max_segments() = 1024][6] i32: an image's segments in
 *                   ascending v, each {v, area, x, y, width, height} with the tight pixel box (first and last non-empty column and
 *                   row).  Segments of ignoreInEval labels are not listed; a stuff label with an instance part (7001) is.  Rows from
 *                   seg_count[b] on are not written.
 * A null output is not computed.  The pixel outputs and ws must be 16-byte aligned.  H * W < 2^31.
 * Legal values: [0, 34) and [1000, 34000).  Integers only - two runs of a call give the same bits.  Never silent: the first word
 * of the workspace is a sticky status word, ORed with
 *   PF_GTPREP_STATUS_FULL   an image has more listed segments than the list holds
 *   PF_GTPREP_STATUS_VALUE  a value in [34, 1000), a label of 34 or more, or a negative or wide i32 / i64 value (compared in the
 *                           map's own width: 2^33 + 7 is illegal)
 * and an image flagged with either lists zero segments (its illegal pixels are written as void: black, 255); the other images of
 * the batch are untouched.  The caller zeroes the first 256 bytes of a fresh workspace once (pf_gt_prepare_status_reset enqueues
 * that); everything else is zeroed by every call with the library's own fill kernel, so a captured call holds kernel nodes only.
 * pf_gt_prepare enqueues only (3 launches: fill, stream, finish); B == 0 launches nothing.  pf_gt_prepare_status copies the status
 * word to the host and waits for the stream.
 */
#define PF_GTPREP_STATUS_FULL 1u
#define PF_GTPREP_STATUS_VALUE 2u
int pf_gt_prepare_workspace(int B, size_t *bytes);
int pf_gt_prepare_max_segments(void);
int pf_gt_prepare(const void *inst, int inst_kind, int B, int H, int W, uint8_t *out_rgb, uint8_t *out_train, uint8_t *out_train_nofg,
                  int *seg_count, int *segs, void *ws, size_t ws_bytes, void *stream);
int pf_gt_prepare_status(const void *ws, void *stream, int *host_status);
int pf_gt_prepare_status_reset(void *ws, void *stream);

/* ------------------------------------------------------------------------------------------
 * pf_bg_dense_input - the network input of BGModel.forward (models/bg/bg_model.py:61-69) for the configurations the fused stem
 * of pf_bg_forward does not cover (convert2onehot = False, or no depth channels): writes x [B, T*C (+T), H, W] f32 for
 * pf_hardnet_forward_dense.
 *   frames   kind 0: labels u8 [B,T,H,W], kind 1: labels i64 [B,T,H,W] (one-hot over `channels` classes, labels >= channels ->
 *            zero vector, :53-59), kind 2: f32 [B,T,channels,H,W] (copied: the reshape of :63-64)
 *   depth    f32 [B,T,H,W] or NULL (use_depth_inps false); depth_mask u8 [B,T,H,W]: channel T*C + t = (depth - mean) / std * mask (:66-69)
 */
int pf_bg_dense_input(const void *frames, int kind, int channels, const float *depth, const uint8_t *depth_mask, float depth_mean,
                      float depth_std, int B, int T, int H, int W, float *x, void *stream);

/* ------------------------------------------------------------------------------------------
 * Validation loss of the bg model (forward part) - replaces BGModel.loss (bg_model.py:73-89):
 * nn.CrossEntropyLoss(ignore_index) of the bilinearly upsampled (align_corners, hardnet.py:372-384) logits and the
 * accuracy counters, fused: the full-resolution logits are never materialised.
 *   logits [B,C,Hin,Win] f32 (the network's orig_size_logits, C = 11 or 19)   labels [B,out_h,out_w] i64 or u8
 *   out3 (device) = { sum over valid pixels of -log softmax(logits)[label], #valid pixels, #pixels with argmax == label }
 *   => loss = out3[0]/out3[1], accuracy = out3[2]/out3[1].  Deterministic (fixed-order fp64 reduction).
 * Workspace: pf_seg_loss_workspace(B, out_h, out_w).  (The training step - this loss with its backward pass - is
 * pf_train_forward_backward below.)
 */
int pf_seg_loss_workspace(int B, int out_h, int out_w, size_t *bytes);
int pf_seg_loss(const float *logits, int B, int C, int Hin, int Win, const void *labels, int labels_i64, int out_h,
                int out_w, int ignore_index, double *out3, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * fg forecaster network - replaces FGModel.forward (models/fg/fg_model.py:216-339) of the shipped fg config
 * (pretrained_models/fg/config.yaml: rnn_type gru, 2 ConvLSTM layers, 2 trajectory output layers, depth + odometry
 * inputs); its pieces: ConvLSTMCell (convlstm.py:44-70), nn.GRU, MaskRCNNConvUpsampleHead.forward
 * (mask_rcnn_conv_upsample_head.py:60-65), _compute_traj_inst_feats (:206-214), _normalize_traj (:179-188) and
 * expand_traj_mask (model_utils.py:11-27).  csrc/fg_net.h lists the units: fg_schedule.cpp decides every launch of a forward and its
 * buffers on the host (pf_debug_fg_schedule below shows the table), fg_net.hip enqueues them, fg_gemm.hip / fg_traj.hip / fg_pack.hip
 * hold the kernels.
 *   flags      0 or PF_FG_PAIR (any other bit: PF_EUNSUPPORTED; reserved for the configuration switches).  The same value goes to
 *              pf_fg_weights_size, pf_fg_pack and pf_fg_forward of one model.
 *   PF_FG_PAIR the eight 3x3 GEMMs (the four ConvLSTM cells, mask_fcn1..4) run on v_mfma_f32_16x16x32_f16: every fp32 operand is
 *              fed as two round-to-nearest fp16 terms, hi = fp16(x), mid = fp16(x - hi), three products hi*hi + hi*mid + mid*hi,
 *              fp32 accumulation (the arithmetic of the bg network's option "split_f16").  Everything in memory stays fp32 and
 *              every other kernel keeps its fp32 code; flags = 0 is untouched.  Unflagged operand bound:
 *              |x - hi - mid| <= 2^-23 |x| + 2^-25; the dropped product is <= 2^-22 of a product.
 *              - packed buffer: the flags = 0 layout followed by a pair section (the fp16 terms of w * 2^k per GEMM, max |w * 2^k|
 *                in [2^14, 2^15), k found on the device; 2^-k is applied in the bias addition, both exact).  A buffer packed with
 *                PF_FG_PAIR is therefore also valid for a flags = 0 forward.  The reverse - a flags = 0 buffer handed to a
 *                PF_FG_PAIR forward - reads past its end: it is the CALLER'S CONTRACT never to do that, nothing checks it.
 *              - workspace: pf_fg_pair_workspace, NOT pf_fg_workspace - that call keeps refusing every non-zero flags value, as
 *                its callers and tests/test_fg_host.py have always had it, so the pair workspace has a size call of its own:
 *                PF_FG_STATUS_BYTES of status block in front of the flags = 0 workspace.  Word 0: PF_STATUS_* bits of the
 *                running forward, zeroed by the forward's first launch (a kernel node; no launch is added beyond that one).  Word
 *                1: OR over the forwards since the host cleared it.  The caller clears the block once after allocating the workspace
 *                (pf_fg_status_reset).  PF_STATUS_RANGE: a staged operand was not <= 65504 in magnitude (NaN included).
 *                PF_STATUS_RANGE_LOW: a K source (traj_feat vector, input planes, h) of one launch had a non-zero maximum
 *                below 2^-6, where the absolute 2^-25 dominates.  All-zero tensors raise nothing; nothing is ever clamped.  A
 *                flagged forward's outputs are not to be used: run it again with flags = 0, or fail.
 *              - pf_fg_status(ws, out2, stream): out2 (host) = {word 0, word 1} with the last forward's RANGE_LOW folded in, both
 *                words cleared; one small kernel, a copy and a SYNCHRONISATION of `stream` - the only fg call that waits, never
 *                made by pf_fg_forward, which stays enqueue-only and capturable.  After replays of a captured forward read word 1.
 *   pf_fg_weights_size: raw = the 52 state_dict tensors of the reference, flattened and concatenated in its state_dict
 *              order (fp32); packed = the device buffer pf_fg_pack fills (raw copy + ConvLSTM / mask head weights re-tiled,
 *              the i, f, o, g rows of 16 hidden channels side by side).  Both in floats.
 *   pf_fg_pack(raw, packed): device buffers; enqueued on stream.  Re-run after the parameters change.
 *   pf_fg_forward: N instances, T_in input steps, T_out = num_output_steps, odom_T >= T_in + T_out steps of odometry:
 *     trajs [N,T_in,8] f32   traj_mask, vel_mask [N,T_in] f32 (0/1)   feats [N,T_in,256,14,14] f32
 *     output_inds [N] i64 (clamped into [0,T_out))   odom [N,odom_T,5] f32   depths [N,T_in,2] f32
 *     depth_mask [N,T_in] f32 (0/1)   classes [N] i64 (clamped into [0,8))
 *   -> traj_norm, traj_unnorm [N,1+T_out,10]   mask_feats [N,1+T_out,256,14,14]   output_feats [N,256,14,14]
 *      masks [N,28,28] (the logits of each instance's class row only, :335-336)
 *   N = 0 enqueues nothing.  Dimensions are checked before any device work.  Workspace: pf_fg_workspace.
 */
#define PF_FG_PAIR 1
#define PF_FG_STATUS_BYTES 1024
int pf_fg_weights_size(int flags, size_t *raw_floats, size_t *packed_floats);
int pf_fg_pack(const float *raw, float *packed, int flags, void *stream);
int pf_fg_workspace(int N, int T_in, int T_out, int flags, size_t *bytes);
int pf_fg_pair_workspace(int N, int T_in, int T_out, size_t *bytes);
int pf_fg_forward(const float *packed, int flags, int N, int T_in, int T_out, int odom_T, const float *trajs,
                  const float *traj_mask, const float *vel_mask, const float *feats, const int64_t *output_inds,
                  const float *odom, const float *depths, const float *depth_mask, const int64_t *classes,
                  float *traj_norm, float *traj_unnorm, float *mask_feats, float *output_feats, float *masks,
                  void *ws, size_t ws_bytes, void *stream);
int pf_fg_status(void *ws, unsigned *out2, void *stream);
int pf_fg_status_reset(void *ws, void *stream);

/* ------------------------------------------------------------------------------------------
 * odometry forecaster network - replaces OdomModel.forward (models/odom/odom_model.py:79-106) of the shipped odom config
 * (pretrained_models/odom/config.yaml: normalize_input, rnn_hidden 128, no inp_emb_layers / out_layers):
 * nn.GRU(2, 128) + Linear(128, 2) on normalised [speed, yaw_rate].  csrc/odom_net.hip, one launch per forecast.
 *   flags      bit 0: predict_type offset (current = current + out); clear: direct (current = out).  Other bits:
 *              PF_EUNSUPPORTED.
 *   pf_odom_weights_size: raw = the 8 state_dict tensors of the reference (odom_mean, odom_std, rnn.weight_ih_l0,
 *              rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0, out.0.weight, out.0.bias), flattened and concatenated in
 *              that order (fp32, 50 950 floats); packed = the device buffer pf_odom_pack fills (raw copy + W_hh re-tiled,
 *              the r, z, n rows of 16 hidden units side by side).  Both in floats.
 *   pf_odom_pack(raw, packed): device buffers; enqueued on stream.  Re-run after the parameters change.
 *   pf_odom_forward: B sequences, T_in input steps (the GRU runs over the first T_in - 1, the decoder starts from the
 *              last), T_out forecast steps:
 *     inps [B,T_in,2] f32 (unnormalised)  ->  out [B,T_out,2] (unnormalised), out_norm [B,T_out,2] (normalised)
 *   Dimensions are checked before any device work: B >= 0, 2 <= T_in <= 64, 1 <= T_out <= 64, no null buffer when B > 0
 *   (PF_EINVAL).  B = 0 enqueues nothing.  No workspace: the state lives in LDS and registers.
 */
int pf_odom_weights_size(int flags, size_t *raw_floats, size_t *packed_floats);
int pf_odom_pack(const float *raw, float *packed, int flags, void *stream);
int pf_odom_forward(const float *packed, int flags, int B, int T_in, int T_out, const float *inps, float *out,
                    float *out_norm, void *stream);

/* ------------------------------------------------------------------------------------------
 * odometry forecaster, training - OdomModel.loss (odom_model.py:104-115) differentiates the forward above; the loss
 * arithmetic on [B,T_out,2] stays with the caller.  csrc/odom_train.hip.
 *   pf_odom_train_workspace: bytes of the buffer both calls below share (what the forward keeps per step, sequence and
 *              hidden unit - h, r, z, n, W_hn h + b_hn - plus the weight-gradient partials); grows with B and with
 *              T_in - 1 + T_out.  0 for B = 0.
 *   pf_odom_train_forward: pf_odom_forward's out / out_norm bit for bit, and the saved state in ws.
 *   pf_odom_backward: grad_out, grad_out_norm [B,T_out,2] f32 = the gradients of a scalar with respect to out / out_norm
 *              (either may be null = zero); ws = the workspace the matching pf_odom_train_forward filled (the call
 *              consumes it: one backward per forward).  grad_raw [50 950] f32 in the raw layout of pf_odom_weights_size
 *              is overwritten (never accumulated); the odom_mean / odom_std slots are written as zero.  No gradient
 *              is produced for inps.
 *   Three kernel launches (reverse sweep, weight gradients per range of (step, sequence) rows, fixed-order sum of the
 *   ranges), no atomics: two runs give the same bits.  Dimensions, null buffers and ws_bytes are checked before any
 *   device work as in pf_odom_forward.  B = 0: the forward enqueues nothing, the backward only the zero fill of grad_raw.
 */
int pf_odom_train_workspace(int B, int T_in, int T_out, int flags, size_t *bytes);
int pf_odom_train_forward(const float *packed, int flags, int B, int T_in, int T_out, const float *inps, float *out,
                          float *out_norm, void *ws, size_t ws_bytes, void *stream);
int pf_odom_backward(const float *packed, int flags, int B, int T_in, int T_out, const float *inps, const float *out_norm,
                     const float *grad_out, const float *grad_out_norm, void *ws, size_t ws_bytes, float *grad_raw,
                     void *stream);

/* Process-wide execution options (not thread-safe; set before launching work):
 *   "fuse_pool"     (default 1) a 1x1 conv followed by AvgPool2d(2,2) (hardnet.py:296) pools in the conv epilogue;
 *   "fuse_upsample" (default 1) TransitionUp + 1x1 conv over cat([up(x), skip]) (hardnet.py:248-258,365-368) is
 *                   evaluated as W_skip*skip + up(W_x*x): same result up to fp32 rounding, no upsampled tensor;
 *   "use_tuned_table" (default 1) per-layer kernel shapes come from the measured table (csrc/conv_tuned.inc) where it
 *                   has the shape, else from the cost model; 0 = cost model only (tools/tune_convs.py);
 *   "split_f16"     (default 1; "split_bf16", its name while the terms were bf16, is still accepted) the table may select
 *                   the split kernels (conv_split, conv_s4) for stride-1 3x3 and 1x1 layers: every fp32 operand split into
 *                   two fp16 terms hi + mid (22 significand bits; weights pre-scaled by an exact power of two per conv),
 *                   three products on v_mfma_f32_16x16x32_f16, fp32 accumulation - single layers within 2e-5*(1+max|ref|)
 *                   of fp64 like the fp32 kernels, whole-network logits within 1e-4 either way.  Operand bound: both terms
 *                   are rounded to nearest even, |x - hi - mid| <= 2^-23 |x| + 2^-25 for |x| <= 65504 (fp32 itself: 2^-24 |x|);
 *                   beyond 65504 the forward raises PF_STATUS_RANGE, and a tensor whose largest value is below 2^-6 (where the
 *                   absolute term would dominate) raises PF_STATUS_RANGE_LOW (above) - never a silent loss in either direction;
 *                   0 = every convolution on fp32 MFMA / fp32 VALU;
 *   "normalize_ranges" (default 1; process-wide only, read when a plan is created) every activation channel is stored
 *                   multiplied by a power of two chosen from the folded weights so that its expected magnitude is 8 (producer
 *                   rows * s, consumer columns / s: bit-identical fp32 arithmetic, fp16-pair range centred on the data; a
 *                   checkpoint re-parameterised across a BatchNorm runs on the same stored values); 0 = store raw values;
 *   "range_guard"   (default 1) the PF_STATUS_RANGE checks of the split path (a compare per stored value); 0 removes them;
 *   "fuse_front"    (default 1) base.1 (3x3 s1, 16 -> 24) and base.2 (3x3 s2, 24 -> 32) as ONE kernel on a packed-pair stem output, the
 *                   tensor between them kept in LDS (csrc/conv_front.hip: workgroups march down 31-column strips): same results
 *                   (tests/test_gpu_bg_model.py), 39 % fewer front-end bytes, 0.42 ms against 0.83 ms for the two separate kernels
 *                   per 16 frames at 1024x2048; 0 = stem -> conv_split -> conv_dma stride 2;
 *   "profile_tag_ops" (default 0; process-wide only) pf_profile_* records carry one label per op of the table (tools/);
 *   "upsample_bwd_two_pass" (default 1; read by pf_train_forward_backward) the transposed bilinear interpolations of the training
 *                   step (the loss head's 4x above all) as a row pass and a column pass over a scratch tensor when the planes are
 *                   large - the one-pass kernel's own nesting and order, so the same bits; 0 = always one pass;
 *   "train_side_stream" (default 1; process-wide only, read by pf_train_create) the weight gradients of the training step - leaves
 *                   of the backward pass - run on the training plan's own lower-priority stream, forked from and joined to the
 *                   caller's stream inside every pf_train_forward_backward (a stream capture of the call stays one graph; the
 *                   results are bit-identical, the workspace grows by one dy slot); 0 = everything on the caller's stream;
 *   "train_table_batch" (default 0; process-wide only, read by pf_train_forward_backward) n > 0: the measured shape table of the
 *                   training step's convolutions (csrc/train_tuned.inc, keyed on the batch it was measured at) is consulted as if
 *                   the batch were n - the kernels of the timed configuration (n = 8) on a batch a CPU checker can afford;
 *   "fuse_pairs"    (default 1) an odd HarDBlock layer computed INSIDE its consumer where both read / write packed pairs
 *                   (csrc/conv_pair.hip: one launch per pair, the shared input staged once, the odd layer kept in LDS planes; the
 *                   (<= 12) -> (17..20)-channel pairs in the MERGED form, the odd layer's weights in the rows the consumer's second
 *                   cout tile pads with zeros): 1 = where it measured faster (launches of 65k-196k pixels), 0 = never, 2 = wherever
 *                   the kernel exists, 3 = everywhere and never merged, 4 = the merged pairs only (A/B runs, tests); results agree
 *                   with the two launches within 1e-5 (1 + max) (tests/test_gpu_conv.py);
 *   "share_s"       (default 1) an odd HarDBlock layer's launch also sums its consumer's rows over the input both read (csrc/conv_s4.hip,
 *                   conv_s4_share_kernel: the odd layer's couts rounded up to 4, then the consumer's, in common cout tiles), and the
 *                   consumer's launch runs over its other ranges and adds the stored sums before bias and ReLU (conv_s4_add_kernel):
 *                   the common input is read once and the consumer's padding rows do the work.  1 = where it measured faster
 *                   (csrc/conv_select.cpp::share_wanted), 0 = never - and a plan CREATED while the process-wide value is 0 packs no
 *                   weights for it -, 2 = wherever the two forms exist (A/B runs, tests); the workspace grows by one scratch region
 *                   of the largest such consumer (fp32); results agree with the two plain launches within 1e-5 (1 + max)
 *                   (tests/test_gpu_share_s.py);
 *   "fold_final"    (default 1) a 3x3 packed-pair conv of two cout tiles whose slice has exactly one reader - the next op, a 1x1 conv
 *                   of at most 16 couts without ReLU into fp32 whose other channels (at most 32, in front of the slice, both starting
 *                   on a 4-channel boundary) were stored earlier - also computes that conv (csrc/conv_s4.hip, conv_s4_tail_kernel): its
 *                   finished values stay in registers as the fp16 pair the reader would load, are multiplied by the reader's weights
 *                   after the centre pixels of the reader's other channels, and the reader's output is stored; the slice never is,
 *                   the reader's launch goes away, and pf_hardnet_tensor_read of the tensor the slice belongs to is refused
 *                   ("elided").  In FC-HarDNet-70: the last decoder layer and finalConv.  1 = where it measured faster
 *                   (csrc/conv_select.cpp::tail_wanted), 0 = never - and a plan CREATED while the process-wide value is 0 packs no
 *                   weights for it -, 2 = wherever the form exists (A/B runs, tests); results agree with the two launches within
 *                   1e-5 (1 + max) (tests/test_gpu_fold_final.py);
 *   "fold_down"     (default 1) a 3x3 packed-pair conv of two cout tiles in front of a 1x1 conv with ReLU of at most 64 couts and that
 *                   conv's 2x2 average pool - the 1x1 conv's single range ends with the 3x3 conv's slice, its other channels (at most 32,
 *                   in front of the slice, both starting on a 4-channel boundary) were stored earlier - also computes the 1x1 conv
 *                   and the pool (csrc/conv_s4.hip, conv_s4_down_kernel): its finished values are stored as ever (other ops may read
 *                   them) and, still in registers as the fp16 pair the reader would load, are multiplied by the reader's weights after
 *                   the centre pixels of the reader's other channels; the pooled output is stored as packed pairs and the reader's
 *                   launch goes away.  In FC-HarDNet-70: base.4.layers.3 and base.5.  1 = where it measured faster
 *                   (csrc/conv_select.cpp::down_wanted), 0 = never - and a plan CREATED while the process-wide value is 0 packs no
 *                   weights for it -, 2 = wherever the form exists (A/B runs, tests); results agree with the two launches within
 *                   1e-5 (1 + max) (tests/test_gpu_fold_down.py).  The same option covers 3x3 convs of three cout tiles, all in one
 *                   workgroup, in front of a 1x1 conv of at most 96 couts (conv_s4_down_kernel<3, 32, 8, 1>, fragments in a region of
 *                   their own; in FC-HarDNet-70: base.7.layers.3 and base.8; tests/test_gpu_fold_wide.py);
 *   "fold_lo"       (default 1) a 3x3 packed-pair conv of three cout tiles in front of an upsample + 1x1 conv pair that runs commuted
 *                   ("fuse_upsample"): the launch also computes the 1x1 conv's columns over the upsample's input at the low resolution
 *                   (at most 64 couts; no bias, no ReLU: those belong to the other half) into the fp32 scratch the other half samples
 *                   (csrc/conv_s4.hip, conv_s4_lo_kernel); the range the upsample reads ends with the 3x3 conv's slice as for
 *                   "fold_down".  The slice is stored only if another op reads it; otherwise pf_hardnet_tensor_read of its tensor is
 *                   refused ("elided").  In FC-HarDNet-70: denseBlocksUp.2.layers.3 and conv1x1_up.3.  0 / 1 / 2 as for "fold_down"
 *                   (csrc/conv_select.cpp::lo_wanted; tests/test_gpu_fold_wide.py);
 *   "train_blocked_sum" (default 1; process-wide only) the 3x3 convolutions of a training step add every round of 8 input channels
 *                   into a second accumulator set (blocked summation, like ATen's): forward activations 0.79-0.95 x as far from
 *                   float64 as torch-CPU fp32; 0 = one fp32 chain over all 9 Cin terms;
 *   "train_forward_s4" (default 0; process-wide only, read by pf_train_create) 1 = the forward 3x3 stride-1 and 1x1 conv +
 *                   BatchNorm layers of a training step run on the packed-pair kernels of the inference path (csrc/train_s4.hip:
 *                   weights packed on the device every step with the fixed scale 2^12 - a weight of magnitude >= 16 becomes NaN,
 *                   loudly - activation slices shadowed as fp16 pairs, fp32 outputs; the 3x3 layers on conv_s4_blocked_kernel, which
 *                   sums every round of 8 input channels on its own like the fp32 step): the step 14.45 -> 14.24 ms at batch 8 of
 *                   800x800, the forward pass 0.81-0.95 x as far from float64 as torch-CPU fp32 (fp32 step: 0.79-0.95 x; without
 *                   the blocked sums 14.0 ms and 1.0-1.2 x); 0 = conv_dma on the fp32 matrix instruction;
 *   "wgrad_taps"    (default 1; process-wide only) weight gradients of 3x3 stride-1 layers with the taps folded into the matrix rows
 *                   (csrc/wgrad_taps.hip: rows = (cout, tap) pairs, 10 outputs fill 90 of 96 rows instead of 10 of 16): 1 = per layer
 *                   where it measured faster, 0 = never (wgrad_tiled_kernel), 2 = wherever the kernel exists; same fixed-order
 *                   partial sums either way (a step stays bit-reproducible), other rounding than the tiled kernel's;
 *   "valu_remainder" (default 1) trailing cout % 16 <= 8 channels of a conv_dma layer on the vector ALU. */
int pf_set_option(const char *name, int value);
/* The same options per plan: a plan copies the process-wide values when it is created; this call changes them for
 * that plan only (read at forward time by forwards of that plan; a plan is used from one thread at a time).  One more
 * name exists only here:
 *   "table_batch"   (default 0) n > 0: the per-layer kernel table is consulted as if every forward had a batch of n —
 *                   a frame's logits then do not depend on how many frames share the call (the tuned table is keyed on
 *                   the batch size, and the split and fp32 kernels differ in the last bits). */
int pf_hardnet_plan_set_option(pf_plan *plan, const char *name, int value);

/* ------------------------------------------------------------------------------------------
 * bg training step (scope row f4) — replaces, per batch, training/train.py:185-222 for task `bg`:
 *   loss_dict = model.loss(inputs, labels)  (bg_model.py:73-89: train-mode BatchNorm, F.interpolate align_corners,
 *   CrossEntropyLoss(ignore_index=255), accuracy) ; loss.backward() ; clip_grad_value_/clip_grad_norm_ ; SGD step.
 *
 * A pf_train is built from the same blob as a plan (only the op table is used).  Parameters are ONE flat fp32 device
 * array `theta`; per conv op of the table, in table order:  W[cout][cin][k][k], then gamma, beta, running_mean,
 * running_var [cout each] for conv+BatchNorm layers (hardnet.py:16-25) or bias[cout] for a plain conv (finalConv).
 * `grad` has the same layout (the running-stat slots stay 0).  pf_train_param_layout gives the offsets of one op.
 *
 * pf_train_forward_backward: forward in training mode (batch statistics; running stats updated in theta when
 * update_running_stats), loss, backward.  Inputs either as the reference batch (seg [B,T,H,W] u8/i64 trainIds, depth,
 * depth_mask, depth_mean/std: one-hot + normalised masked depth built on the device, bg_model.py:53-69) or as a dense
 * x_dense [B,in_ch,H,W].  labels [B,out_h,out_w] u8/i64.  grad is zeroed first unless accumulate_grads (train.py's
 * accumulate_steps; loss_scale = 1/accumulate_steps multiplies the gradient).  out3 (device, 3 doubles) = {sum of the
 * per-pixel losses, number of labels != ignore_index, number of correct argmax}: loss = out3[0]/out3[1], accuracy =
 * out3[2]/out3[1].  Only enqueues on `stream`; every reduction runs in a fixed order (bit-reproducible).
 *
 * pf_sgd_step: g *= min(1, clip_norm/(||g||+1e-6)) if clip_norm > 0 (clip_grad_norm_); clamp to +-clip_value if > 0
 * (clip_grad_value_); g += weight_decay*p; buf = first_step ? g : momentum*buf + g; p -= lr*buf (torch.optim.SGD) on
 * the elements with trainable[i] != 0 (the running statistics are buffers, not parameters).  For data-parallel
 * training all-reduce `grad` (one RCCL call, ~16.5 MB) between the two calls (reference: DDP, train.py:96-103). */
typedef struct pf_train pf_train;
int pf_train_create(const void *blob, size_t blob_bytes, int in_ch, int n_cls, pf_train **out);
void pf_train_destroy(pf_train *t);
/* enable != 0: the workgroup shape of every forward / backward-data convolution is measured (all candidates, a few launches
 * each, hipEvents + a stream synchronisation) in a pass of its own in front of the first pf_train_forward_backward of a
 * configuration (B, H, W, out size) that runs outside a stream capture - that pass leaves theta, grad and the running statistics
 * alone - then kept for the life of the plan; 0 (default): the shapes of csrc/train_tuned.inc / the cost model, and the measured
 * ones are forgotten.  Call it before pf_train_workspace: the measuring pass needs n_params floats more.  The measured choice depends on
 * timing: with it, two runs need not pick the same summation order for the K-split shapes (results equal to rounding, not
 * to the bit, from run to run; within one plan they are reproducible once every geometry has been seen). */
int pf_train_autotune(pf_train *t, int enable);
/* what pf_train_autotune has measured so far: rows of 10 ints {ks, stride, Cin, Cout, Hin, Win, B, accumulate, pixel waves,
 * cout tiles} ({.., 0, 0} = the cost model's own shape won); *n_rows = rows available, at most cap_rows are written.
 * tools/tune_train.py turns them into csrc/train_tuned.inc, the table plans that do not measure consult (option "use_tuned_table"). */
int pf_train_tuned_shapes(const pf_train *t, int *rows, int cap_rows, int *n_rows);
/* which code paths the LAST pf_train_forward_backward of this plan took: stats[0] convolutions launched with a row of
 * csrc/train_tuned.inc, [1] with the cost model's shape, [2] with a shape pf_train_autotune measured, [3] odd-width convolutions
 * run on row-padded copies (gather), [4] of those, forward conv + BatchNorm layers whose output stayed in padded rows, [5]
 * odd-width layers whose input gradients came from ONE backward-data conv over all ranges, [6] launches of the generic
 * (register-staged) kernel, [7] forward convolutions run on the packed-pair kernels (option "train_forward_s4").  *n = 8 values
 * available, at most cap are written.  (Tests: the timed configuration's kernels ran.) */
int pf_train_path_stats(const pf_train *t, int *stats, int cap, int *n);
int pf_train_param_count(const pf_train *t, size_t *n_floats);
int pf_train_param_layout(const pf_train *t, int op_index, size_t *w_off, size_t *aux_off, int *has_bn);
int pf_train_workspace(const pf_train *t, int B, int H, int W, int out_h, int out_w, size_t *bytes);
int pf_train_forward_backward(const pf_train *t, float *theta, float *grad, int accumulate_grads, const void *seg, int seg_is_i64,
                              const float *depth, const uint8_t *depth_mask, float depth_mean, float depth_std, int T,
                              const float *x_dense, int B, int H, int W, const void *labels, int labels_i64, int out_h, int out_w,
                              int ignore_index, float loss_scale, float bn_momentum, float bn_eps, int update_running_stats,
                              double *out3, void *ws, size_t ws_bytes, void *stream);
/* where tensor `name` (activation, or its gradient with want_grad) lives in the training workspace (tests) */
int pf_train_tensor_view(const pf_train *t, const char *name, int want_grad, int B, int H, int W, int out_h, int out_w,
                         size_t *ws_offset, int *channels, int *h, int *w);
int pf_sgd_workspace(size_t *bytes);
int pf_sgd_step(float *theta, float *grad, float *momentum_buf, const uint8_t *trainable, size_t n, float lr, float momentum,
                float weight_decay, float clip_norm, float clip_value, int first_step, void *ws, size_t ws_bytes, void *stream);

/* Introspection for per-stage parity tests: where tensor `name` (packing.py tensor names, e.g.
 * "base.4.out") lives inside the workspace for this (B,H,W): byte offset, channels, height, width. */
int pf_hardnet_tensor_view(const pf_plan *plan, const char *name, int B, int H, int W,
                           size_t *ws_offset, int *channels, int *h, int *w);
/* Copy tensor `name` of the LAST forward of this plan out of its workspace as fp32 NCHW [B,channels,h,w].  Intermediate
 * tensors may live in the packed-pair layout of conv_s4.hip (plan option "packed_acts", on by default): two fp16 terms
 * hi = fp16(x), mid = fp16(x - hi) (round to nearest even) per element in [B][2][ceil(C/4)][H][W][4] order - this call undoes it. */
int pf_hardnet_tensor_read(const pf_plan *plan, const char *name, int B, int H, int W, const void *ws, float *dst, void *stream);
/* fp32 NCHW <-> packed-pair layout (dst of pf_s4_pack: 16 * B * ceil(C/4) * H * W bytes); tests and tensor taps.
 * status (nullable, device word): PF_STATUS_RANGE is raised when an element is not representable (|x| > 65504, NaN). */
int pf_s4_pack(const float *src, void *dst, int B, int C, int H, int W, unsigned *status, void *stream);
int pf_s4_unpack(const void *src, float *dst, int B, int C, int H, int W, void *stream);
/* Dense-equivalent FLOPs of one forward at (H,W) per sample (2*Cout*Hout*Wout*Cin*k*k summed). */
int pf_hardnet_flops(const pf_plan *plan, int H, int W, double *flops);

/* ------------------------------------------------------------------------------------------
 * Opt-in per-launch timing for the roofline report (bench.py).  While enabled, every kernel the
 * library enqueues is bracketed by hipEvents on ITS launch stream (process-wide state; do not
 * enable during graph capture).  pf_profile_collect() synchronises the recorded events and returns
 * the number of distinct kernels; pf_profile_get() returns, per kernel (label = the demangled
 * symbol rocprofv3 prints), launches, summed duration and the summed ALGORITHMIC flops / bytes of
 * those launches (SURVEY.md 8d accounting: unique input + output bytes; 2*Cout*H*W*Cin*k*k flops).
 */
int pf_profile_enable(int on);
int pf_profile_collect(void);
int pf_profile_get(int i, char *label, size_t label_cap, int *launches, double *total_ms, double *flops,
                   double *bytes);

/* Tuning/diagnostic hook (tools/tune_convs.py, tools/tune_s4.py, tests): force the convolution kernel and tile shape of every
 * stride-1 conv the library launches from now on.  kind (csrc/conv_mfma.h: ConvKind) 0 = CONV_AUTO, automatic (default);
 * 1 = CONV_DMA, conv_dma (p0 = WM in {1,2,4}, p1 = NT; 0 = by its cost model); 2 = CONV_WAVE, conv_wave (p0 = rows per tile in
 * {1,2,4}, p1 = NT in {1,2}, p2 = K-split waves in {2,4,8,16}); 3 = retired (was conv_valu); 4 = CONV_SPLIT, conv_split (p0 = NT in
 * {1,2,3}, p1 = 1 for 8x64-pixel tiles); 5 = CONV_S4, conv_s4 on packed-pair sources wherever the plan can provide them, conv_dma
 * elsewhere (p0 = NT, p1 = the 3x3 pixel tile, S4Tile: 0 = S4_8x32, 1 = S4_8x64, 2 = S4_16x32, 3 = S4_8x32_K2, 4 = S4_8x32_K4 - 8x32
 * with 2 / 4 wave groups splitting the K rounds).  Shapes that are not built fall back to the automatic choice.  Process-wide, not
 * thread-safe.
 * The training step honours kind 1 only: while pf_debug_force_conv(1, wm, nt, 0) is set, every forward and backward-data
 * convolution of pf_train_forward_backward (stride 2 included) runs conv_dma with wm pixel waves and min(nt, the layer's cout
 * tiles) cout tiles per workgroup (wm = 1: at most 2; nt = 0: the cost model's count) instead of the shape of csrc/train_tuned.inc,
 * the cost model or pf_train_autotune, and pf_train_path_stats counts it in none of stats[0..2] (tests: every built shape of the
 * training convolutions against a reference). */
int pf_debug_force_conv(int kind, int p0, int p1, int p2);
/* Host only, no device involved, nothing enqueued (tests): what the schedules decide for one convolution (csrc/conv_select.cpp:
 * decide_conv) under the current pf_debug_force_conv.  B = the batch the choice is made for, need: bit 1 = pooling epilogue, bit 2 =
 * another fused stage; flags: 1 = input width % 4 != 0 (generic kernel), 2 / 4 = the plan has the conv_split / conv_s4 packing of the
 * conv, 8 = option use_tuned_table, 16 = option split_f16, 32 = blocked sums (training); rounds = K rounds of the conv_s4 packing.
 * out[0..10] (cap >= 11) = kind, p0, p1, p2 of the fp32-source kernel, whether the conv wants packed-pair sources, the conv_s4 NT and
 * tile it then asks for, and NT, TW, TH, KS of the conv_s4 instantiation that request runs (s4_resolve). */
int pf_debug_conv_decision(int ks, int stride, int cin, int cout, int hout, int wout, int B, int need, int flags, int rounds,
                           int *out, int cap);
/* Host only, no device involved, nothing enqueued (tests): the kernel the library runs for a fused stem (what = 0), an upsample + argmax
 * head (1) or pf_seg_loss (2) of the given sizes (csrc/net_select.cpp), or the error code (and pf_last_error) with which the launch would be
 * refused.  what 0: iargs[11] = T, n_cls, H, W, Hout, Wout, B, seg_is_i64, hop flags, dst_fmt (1 = packed pairs for the fused front end),
 * whether the plan's re-packed stem weights are present; fargs[4] = depth mean, std, min_depth, max_depth.  what 1 and 2: iargs[6] = B, C,
 * Hin, Win, Hout, Wout, no fargs.  label (label_cap bytes, nullable with 0) = the launch's profile label.  out[0..7] (cap >= 8): [0] the
 * family (stem: 0 generic, 1 v3, 2 v4; head: 0 head_kernel, 1 head4_kernel, 2 head_col_kernel), [1..3] grid x, y, z, [4] lanes per
 * workgroup, [5] dynamic LDS bytes, [6] stem: the flags in force, 1 = SEG64, 2 = HOP_D, 4 = HOP_LUT, 8 = FAST_DIV; head: C; loss: workgroups
 * of the tile kernel (= partial sums), [7] stem: the row of the family's instantiation list; loss: the bytes of pf_seg_loss_workspace. */
int pf_debug_net_choice(int what, const int *iargs, int n_iargs, const float *fargs, int n_fargs, char *label, size_t label_cap,
                        long long *out, int cap);
/* Host only, no device involved, nothing enqueued (tests): the range tables of one launch of a convolution that reads n_src (1..4) channel
 * ranges - range j = channels [choff[j], choff[j] + ch[j]) of a tensor of ctotal[j] channels - as the packers and the schedules take them from
 * csrc/conv_ranges.cpp; n_cases convolutions per call: choff, ch, ctotal = [n_cases][4] ints, out = [n_cases][39] (cap ints, >= 39 * n_cases).
 * form: 0 = the op's ranges as they are, 1 = the consumer of a conv_pair launch ([S, others.., P], P at channel 0 of its own planes),
 * 2 = the add launch (without S, the op's range 1); forms 1 and 2 need n_src >= 2.  kc > 0: the tables of a kernel family
 * that walks chunks of kc input channels; kc = 0: the packed-pair tables of a ks x ks conv (ks 1 or 3), pad = every range padded to whole
 * rounds.  0 <= src_begin < src_end <= the launch's ranges: the ranges it accumulates (else all of them).  Per case: [0] ranges of
 * the launch, [1] its chunks (kc > 0) or rounds, [2..5] which range of the op each is, [6..10] src_cstart, [11..14] each range's first input
 * channel in the op's weight numbering, [15..19] src_chunk0, [20..23] src_c4, [24..27] src_g0, [28..31] src_gn, [32..36] src_ent0,
 * [37] chunk_begin, [38] chunk_end; what the chosen tables do not fill is 0. */
int pf_debug_conv_ranges(int form, int ks, int kc, int pad, int n_src, int n_cases, const int *choff, const int *ch, const int *ctotal,
                         int src_begin, int src_end, int *out, size_t cap);
/* Host only, no device involved (tests): one weight layout of csrc/conv_pack.cpp for the OIHW weights w [cout][cin][ks][ks] of a conv that
 * reads n_src (1..4) ranges, range j = ch[j] channels from channel choff[j] of its tensor (sum of ch = cin).  *n_floats = what the layout's
 * size function answers; PF_EINVAL (nothing written) when cap, the floats out has room for, is smaller.  layout: 0 = generic
 * (pack_conv_weights under choose_tiling), 1 = tiled and 2 = rem, the last `rem` (1..16) couts (conv_dma; chunks of dma_kc(ks, stride)),
 * 3 = wave, 4 = split (3x3), 5 = split1 (1x1), 6 = s4 (pad_sources: every range padded to whole rounds), 7 = fold: the 1x1 reader's
 * fragments for `tiles` cout tiles and `chunks` (2 or 3) K chunks, range 0 = the reader's other channels (ch may be 0), range 1 = the
 * slice right behind them, 8 / 9 = the `two` / `nine` stream of conv_pair's producer (3x3, one range).  The fp16-pair layouts (4..9) take
 * the weights as given: already scaled.  Arguments a layout does not take are ignored. */
int pf_debug_pack_conv(int layout, int ks, int stride, int cin, int cout, int n_src, const int *choff, const int *ch, int pad_sources,
                       int rem, int tiles, int chunks, const float *w, float *out, size_t cap, size_t *n_floats);
/* Host only, no device involved (tests): the weight arena a plan created now from this blob would upload - every packing of every
 * convolution under the process-wide options - copied to out when cap >= *n_floats, and per op of the table (table_ops rows of six
 * numbers, nullable): offset in floats and rounds of its packed-pair packing, offset and cout tiles of its share launch's packing,
 * offset and rounds of its add launch's ("share_s"; 0 = the op has none). */
int pf_debug_plan_arena(const void *blob, size_t bytes, int in_ch, int n_cls, float *out, size_t cap, size_t *n_floats,
                        long long *table, int table_ops);
/* Host only, as pf_debug_plan_arena: the region that plan keeps beside its arena for the tail form ("fold_final") - its first 64 floats
 * are zeros, *n_floats = 0 when no op has the form - copied to out when cap >= *n_floats, and per op of the table (table_ops numbers,
 * nullable) the offset in floats of the 1x1 reader's fragments, kept on the 3x3 op: [chunk 2][term 2][lane 64][8 fp16]; 0 = none. */
int pf_debug_plan_tail(const void *blob, size_t bytes, int in_ch, int n_cls, float *out, size_t cap, size_t *n_floats,
                       long long *table, int table_ops);
/* Host only, as pf_debug_plan_tail: the region of the down form ("fold_down"), and per op the offset in floats of the 1x1 reader's
 * fragments, kept on the 3x3 op: [cout tile 4][chunk 2][term 2][lane 64][8 fp16]; 0 = none. */
int pf_debug_plan_down(const void *blob, size_t bytes, int in_ch, int n_cls, float *out, size_t cap, size_t *n_floats,
                       long long *table, int table_ops);
/* Host only, as pf_debug_plan_down: the regions of the forms of three-tile producers - form 2: down3 ("fold_down"), [cout tile 6]; form 3:
 * lo ("fold_lo"), [cout tile 4] - whose fragments are [cout tile][chunk 3][term 2][lane 64][8 fp16] (chunk 2: the third cout tile's
 * four values of a lane in its low half, zeros above). */
int pf_debug_plan_wide(int form, const void *blob, size_t bytes, int in_ch, int n_cls, float *out, size_t cap, size_t *n_floats,
                       long long *table, int table_ops);
/* Host only, no device involved, nothing enqueued (tests): the schedule of one inference forward (csrc/hardnet_schedule.cpp) of the plan
 * a blob would give now under the process-wide options and pf_debug_force_conv, with the per-plan option table_batch as given (0 = the
 * batch itself), on B inputs of H x W.  stem_T > 0: the pf_bg_forward route, a fused stem over stem_T frames; stem_T = 0: the
 * pf_hardnet_forward_dense route.  Weights, fold regions, workspace and the caller's buffers get made-up addresses that are far apart
 * and the same on every call; the schedule computes with them and reads nothing through them.
 * formats: per tensor of the table (*n_formats of them, copied while they fit) what pf_hardnet_tensor_read goes by: 0 = fp32 NCHW,
 * 1 = packed pairs (S4), 0xFF = never stored (the tensor inside the fused front end), 0xFE = its last slice never stored (tail / lo).
 * steps: *n_steps rows of 30 (copied while they fit), one per launch in order (S_STEM_FRONT: the stem and the front end):
 * [0] kind (enum StepKind of csrc/hardnet_schedule.h), [1] first op of the table it executes, [2] op whose weights it runs (-1: not a
 * convolution); [3..6] NT, TW, TH, KS of the conv_s4 instantiation it launches (0 unless kind is one of the S_CONV_S4.. kinds);
 * [7..10] kind, p0, p1, p2 of the ConvChoice of the other convolution kinds (csrc/conv_mfma.h; else 0); [11] src_fmt, [12] dst_fmt,
 * [13] tensor it stores (the fused pool's, the front end's output); [14] fused 2x2 pool, [15] samples a residual, [16] no bias (the
 * low-resolution half of a commuted upsample + 1x1), [17] its own slice is not stored (lo); [18] cout tiles, [19] K chunks / rounds,
 * [20] couts of the folded 1x1 conv, [21] couts of the share / add sums, [22] format of the down form's pooled tensor; [23], [24] the
 * ranges [src_begin, src_end) of op [2] it accumulates (pair, add: the consumer's), [25..28] the tensor of each range of op [2] as the
 * step reads it (-1: none); [29] arg_hash, a 64-bit FNV-1a of its labels and of the argument struct handed to its launcher - equal
 * across calls and builds exactly when every argument is; no meaning of its own.  Columns [11], [12] and [14..28] are 0 / -1 unless the
 * step is a convolution or a pair ([12]: or the front end); [13] is the op's destination for every other step. */
int pf_debug_hardnet_schedule(const void *blob, size_t bytes, int in_ch, int n_cls, int B, int H, int W, int out_h, int out_w, int stem_T,
                              int table_batch, unsigned char *formats, int cap_formats, int *n_formats, long long *steps, int cap_steps,
                              int *n_steps);
/* Host only, no device involved, nothing enqueued (tests): the plan of one pf_train_forward_backward of a training plan created now
 * from this blob - the workspace layout and the schedule of a step on B dense inputs of H x W with labels of out_h x out_w, under
 * the process-wide options as pf_train_create and a step read them, without pf_train_autotune; the addresses it is built against
 * are made up.  *n_regions / *n_steps = rows of the two tables; rows are copied while they fit (cap_regions, cap_steps rows).
 * regions: rows of 4 {kind, index, offset, bytes}, one per workspace region in the order the layout hands them out.  kind: 0
 * activation, 1 gradient, 6 packed-pair shadow (index = tensor); 2 conv output before BatchNorm, 3 batch statistics, 4 gathered
 * row-padded input (index = op); 5 / 7 tiled / packed-pair weight packings; 8 the measuring pass's gradients; 9 dy (index = slot),
 * 10 weight-gradient partial sums (index = side stream), 11 / 12 padded input / output copy, 13 the loss gradient at label size,
 * 14 scratch of the two-pass bilinear transpose, 15 / 16 partial sums of the loss / of BatchNorm, 17 the loss sums; the last row
 * is {18, 0, 0, workspace bytes} = pf_train_workspace.  Offsets are multiples of 256; bytes = what the region was asked to hold.
 * steps: rows of 5.  {0, kind, side stream (-1 = the caller's), dy slot, stats bits} per step of the schedule, in order (kind: TStepKind
 * of csrc/train_plan.h; bit k of the stats bits: the step counts in slot k of pf_train_path_stats), each followed by one row
 * {1, tensor, first channel, channels, access} per channel range of a tensor's gradient buffer the step touches - access 0 = stores,
 * 1 = adds, 2 = clears, 3 = reads - read back from the step's pointers, not from what the builder meant.
 * slots_streams (nullable): {dy slots, side streams} the library was built with. */
int pf_debug_train_plan(const void *blob, size_t bytes, int in_ch, int n_cls, int B, int H, int W, int out_h, int out_w,
                        long long *regions, int cap_regions, int *n_regions, int *steps, int cap_steps, int *n_steps, int *slots_streams);
/* Host only, no device involved, nothing enqueued (tests): the schedule of one pf_fg_forward(flags, N, T_in, T_out) - every launch in
 * order with its buffers (csrc/fg_schedule.cpp) - and the workspace layout.  Refuses what pf_fg_forward refuses (dims, flags).
 * *n_regions / *n_steps = rows of the tables; rows are copied while they fit (cap_regions, cap_steps rows).
 * regions: rows of 3 {region, offset, bytes}, one per workspace region in layout order (region: enum Region of csrc/fg_net.h; the status
 * block comes first and is empty without PF_FG_PAIR); offsets are multiples of 256, bytes = what the region holds; the last row is
 * {0, 0, workspace bytes} = pf_fg_workspace / pf_fg_pair_workspace.
 * steps: rows of 30, read back from the fields the enqueue loop hands to the launchers.  [0] kind (enum StepKind), [1] GEMM id (-1: not
 * a GEMM), [2] epilogue, [3..5] channels of the K sources vec, x, h (h's also where a layer's first cell has no h), [6] ctot of the
 * GEMM's packed weights, [7] pair weight section = scale index, [8] status-slot index (the launch owns words FG_SLOT0 + 3 * index .. + 2;
 * both -1 unless kind = K_PAIR), [9] decoder step (-1: the encoder's launch of the instance feature / trajectory kernels), then for each
 * of vec, x, h, out, c four numbers {region (0 = R_NONE: no such operand), offset, per-instance stride, floats it spans per instance},
 * offset and stride in floats from the region's start; a caller's tensor (R_FEATS ..) is a region.  Instance n's range is [offset +
 * n * stride, + span).  c (the ConvLSTM cell state, the GRU state) is read and written in place.
 * labels (nullable): [cap_steps][64] chars, the NUL-padded profile label of each step ("" = the launch has none). */
int pf_debug_fg_schedule(int N, int T_in, int T_out, int flags, long long *regions, int cap_regions, int *n_regions, long long *steps,
                         char *labels, int cap_steps, int *n_steps);
/* Host only, no device involved, nothing enqueued (tests): how the count kernels of pf_confusion_accumulate and pf_iiou_accumulate
 * (csrc/label_scan.h) split an image of n pixels whose two maps start at addr_a / addr_b, have elements of esz_a / esz_b bytes and
 * are loaded by a lane in units of P pixels that need align_a / align_b bytes of alignment.  out5 = {head, units, tail0, map a
 * aligned after the head, map b aligned after the head}: pixels [0, head) and [tail0, n) are read per element, units * P pixels
 * from head on by unit loads.  head is the fewest pixels below 16 that align both maps, failing that map a alone, clamped to n. */
int pf_debug_label_scan_span(unsigned long long addr_a, unsigned long long addr_b, int esz_a, int esz_b, int align_a, int align_b,
                             unsigned long long n, int P, unsigned long long *out5);
/* Host only, no device involved (tests): row `index` (0 .. 34) of the Cityscapes label table behind pf_gt_prepare (csrc/gt_labels.h).
 * out8 = {id, trainId, category id, hasInstances, ignoreInEval, r, g, b}; name and category are NUL-terminated, cut to their
 * capacities.  PF_EINVAL past the table's end. */
int pf_debug_gt_labels(int index, int *out8, char *name, size_t name_cap, char *category, size_t category_cap);
/* Instrumented builds only (make libpfhip_probe.so, env PF_PROBE=1): the 64 in-kernel timestamps (shader clock)
 * written by workgroup 0 / wave 0 of the last conv_wave launch; PF_EINVAL when nothing was recorded. */
int pf_debug_probe_read(long long *host64);
/* The fill of every destination tile's source-block list after the last pf_warp_splat call that used the workspace `ws` with these
 * dimensions and flags: host_counts[B][G][32x128 destination tiles, row-major], G = T with PF_SPLAT_PER_FRAME and 1 without.  A
 * count is the number of 8x32 source blocks whose valid points' bins touch the tile (above 64 the list overflowed and the tile took
 * the box-scan path).  n_counts receives B*G*tiles; host_counts == NULL only asks for it.  Waits for `stream`. */
int pf_debug_splat_counts(const void *ws, size_t ws_bytes, int B, int T, int H, int W, int per_frame, unsigned *host_counts, size_t cap,
                          size_t *n_counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PFHIP_H */
