/*
 * clairvoyante_amd.h -- C ABI of the MI355X-native Clairvoyante v3 pileup-CNN path.
 *
 * The reference has no FFI layer: its boundary is the duck-typed Python class
 * `Clairvoyante` (clairvoyante/clairvoyante_v3.py:5-284, same surface in
 * clairvoyante_v3_slim.py) whose methods each wrap ONE `tf.Session.run`.  This
 * header is what a binding for that class would bind instead of TensorFlow: every
 * entry point below names the reference method / session.run it replaces.
 * INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - plain C; pointers + sizes only.  `*_dev` pointers are DEVICE (HBM) pointers
 *     (e.g. torch `tensor.data_ptr()`), `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).  Work is enqueued on `stream`; calls do not
 *     synchronise unless stated.
 *   - tensors use the reference's layouts: X [n,33,4,4] fp32 NHWC
 *     (position, base ACGT, matrix), already with matrices 1..3 minus matrix 0
 *     (clairvoyante/utils_v2.py:46); Y [n,16] fp32; parameters in TensorFlow
 *     layouts (conv HWIO, dense [in,out]) keyed by their checkpoint variable names.
 *   - every function returns 0 on success, non-zero on error; cv_last_error()
 *     returns a thread-local message.  No ownership crosses the boundary except
 *     the opaque handle.
 *   - a handle is bound to one GPU and may be used from any host thread, one call
 *     at a time (the reference drives predictNoRT/trainNoRT from a worker thread:
 *     callVar.py:197-204, train.py:87-109).
 */
#ifndef CLAIRVOYANTE_AMD_H
#define CLAIRVOYANTE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CV_INPUT_H 33      /* 2*flankingBaseNum+1, clairvoyante/param.py:6 */
#define CV_INPUT_W 4       /* A C G T */
#define CV_INPUT_C 4       /* matrixNum, clairvoyante/param.py:7 */
#define CV_NUM_OUT 16      /* base4 | zygosity2 | varType4 | indelLength6 */
#define CV_NUM_PARAMS 18

/* Constructor arguments of the reference class (clairvoyante_v3.py:7-16).
 * v3 full: kh {1,2,3} cout {16,32,48} pool {5,4,3} fc4 336 fc5 168
 * v3 slim: kh {1,3,5} cout {8,16,32}  pool {1,1,1} fc4 36  fc5 18
 * (clairvoyante_v3_slim.py:9-11; no pooling layers = window 1).              */
typedef struct cv_arch {
    int32_t kh[3];      /* kernelSize{1,2,3}[0]; the width is always 4        */
    int32_t cout[3];    /* numFeature{1,2,3}                                   */
    int32_t pool[3];    /* pollSize{1,2,3}[0]; 1 = layer absent                */
    int32_t fc4, fc5;   /* hiddenLayerUnits{4,5}                               */
} cv_arch;

typedef struct cv_model cv_model;

/* thread-local text of the last failure on the calling thread */
const char *cv_last_error(void);

/* replaces Clairvoyante.__init__ + _buildGraph + tf.Session (v3.py:7-29):
 * allocates weights, optimizer slots and workspaces on GPU `device`.          */
int cv_create(const cv_arch *arch, int device, cv_model **out);
/* replaces Clairvoyante.close / __del__ (v3.py:180,283) */
int cv_destroy(cv_model *m);

/* Variable table = tf.trainable_variables() of the reference graph
 * (jupyter_nb/visualization.ipynb:103-120).  idx in [0, CV_NUM_PARAMS).       */
int cv_param_info(const cv_model *m, int idx, const char **tf_name, int *ndim, int64_t dims[4]);
/* Flat fp32 device buffer holding all 18 variables back to back in table order
 * (TF layouts): what restoreParameters fills and saveParameters reads
 * (v3.py:243-251), what a data-parallel host all-reduces / broadcasts.
 * `offsets` (optional) receives CV_NUM_PARAMS+1 float offsets.                 */
int cv_param_buffer(cv_model *m, float **flat_dev, int64_t *count, int64_t *offsets);
/* copy one variable in (tf.train.Saver.restore, v3.py:248-251) / out (save).
 * `src`/`dst` are HOST pointers; synchronous with respect to `stream`.        */
int cv_set_param(cv_model *m, const char *tf_name, const float *src, int64_t count, void *stream);
int cv_get_param(cv_model *m, const char *tf_name, float *dst, int64_t count, void *stream);
/* tell the model the flat buffer was modified externally (repack on next use) */
int cv_params_changed(cv_model *m);

/* replaces session.run((YBaseChangeSigmoid, YZygositySoftmax, YVarTypeSoftmax,
 * YIndelLengthSoftmax), phase False) of predict / predictNoRT (v3.py:257-280).
 * out16_dev [n,16]: columns 0..3 base sigmoid, 4..5 zygosity softmax,
 * 6..9 variant-type softmax, 10..15 indel-length softmax.  n may be 0.          */
int cv_forward(cv_model *m, const float *x_dev, int64_t n, float *out16_dev, void *stream);
/* The same pass with the logits where cv_forward leaves the softmaxes -- embedding1..4 of getEmbedding.py:55-57
 * (v3.py:154-158).  out16_dev [n,16]: columns 0..3 the base sigmoid (the bits cv_forward writes there), 4..5, 6..9 and
 * 10..15 selu(FC) + 1e-10f of the zygosity, variant-type and indel-length heads.  Same contract as cv_forward (any n,
 * chunked, asynchronous on `stream`, the same workspace) and, per stage, the same kernel form: the one that computes
 * the heads runs with its logits epilogue, a template argument that cv_kernel_name shows ("heads_tm<true>",
 * "dense_tm<21, 8, 3, 2, true>", ...).  Counts as the last pass for cv_get_activation.                           */
int cv_forward_logits(cv_model *m, const float *x_dev, int64_t n, float *out16_dev, void *stream);
/* selu(conv_layer) BEFORE pooling -- m.conv1..m.conv3 of getTensorAndLayerPNG.py:124-132 -- of all n candidates, into
 * dst_dev in natural layout [n, hc, 4, cout] (full: hc = 33 / 29 / 26; slim, which does not pool: 33, and the values
 * are cv_get_activation 1..3's).  layer 1..3, anything else is an error.  The tile kernels pool the raw accumulators,
 * so this map exists nowhere on their path: per chunk the entry runs the forward pass (which leaves the workspace,
 * cv_kernel_name and cv_get_activation as cv_forward would) and one plain launch over the pooled map below straight
 * into dst_dev, whose chunk the pass first uses for its 16 outputs per candidate.  No model state beyond the pass
 * workspace; candidate offsets in 64 bits.  The inspection path, not the throughput path: the same bits under
 * "impl" 0 and 1.                                                                                                  */
int cv_forward_conv_map(cv_model *m, const float *x_dev, int64_t n, int layer, float *dst_dev, void *stream);

/* Device-side part of callVar.Output (callVar.py:59-72,81-87): per candidate
 * argmax of the three softmax heads (lowest index wins ties, np.argmax), the two
 * best bases of the sigmoid head (highest index wins ties, argsort()[::-1]),
 * the genotype-quality operands (top-2 products, fp32) and the depth sum `dp`.
 * call_dev [n,8] int32: varType, zygosity, indelLength, base1, base2, 0,0,0
 * qual_dev [n,4] fp32 : top1 product, top2 product, dp, 0                       */
int cv_call_postproc(cv_model *m, const float *x_dev, const float *out16_dev, int64_t n,
                     int32_t *call_dev, float *qual_dev, void *stream);

/* Device side of the evaluation report (evaluate.py:78-107, train.EvaluateReport): ADDS what n candidates contribute
 * to counts_dev[64] (int64, on the device, 8-byte aligned; the caller zeroes it):
 *   [0] candidates, [1] top-1 hits, [2] top-2 hits of the base head, [3] unused,
 *   [4..8)   zygosity      2 x 2, row = truth, column = prediction,
 *   [8..24)  variant type  4 x 4,
 *   [24..60) indel length  6 x 6,
 *   [60..64) untouched.
 * out16_dev [n,16] fp32 as cv_forward writes it; y_dev [n,16] labels, fp32 (y_is_f64 == 0) or float64, compared in
 * that type; both 16-byte aligned.  The truth index of a head and the prediction of the three softmax heads are
 * np.argmax (the first maximum; NaN counts as the maximum, the first NaN wins); the base head is ordered as
 * argsort(kind="stable")[::-1] orders it (descending, NaN above every number, of equal values -- +0 and -0 among
 * them -- the higher index first): top-1 counts truth == first, top-2 truth == first or second.
 * No model handle: the kernel runs on the current device, enqueued on `stream`; nothing synchronises or allocates.
 * n == 0 returns 0 and touches nothing; n < 0, a null pointer or a misaligned one returns 1.                        */
#define CV_EVAL_COUNTS 64
#define CV_EVAL_ALL 0
#define CV_EVAL_TOP1 1
#define CV_EVAL_TOP2 2
#define CV_EVAL_ZYGOSITY 4
#define CV_EVAL_VARTYPE 8
#define CV_EVAL_INDEL 24
int cv_eval_counts(const float *out16_dev, const void *y_dev, int y_is_f64, int64_t n, int64_t *counts_dev,
                   void *stream);

/* Host half of callVar.Output (callVar.py:72-153): the VCF records of n candidates from the decisions of
 * cv_call_postproc -- quality int(-4.343*log((p2+1e-300)/(p1+1e-300))), SNP / REF allele, inserted bases and
 * indel-length guess from the tensor, <INS>/<DEL> + SVTYPE, LENGUESS, GT, FILTER, "%.4f" allele fraction -- as text,
 * one '\n'-terminated line per record, in candidate order.  All pointers are HOST pointers.
 *   call [n,8] int32, qual [n,4] fp32: as cv_call_postproc wrote them;
 *   x: tensors [rows,33,4,4] fp32 (matrices 1..3 minus matrix 0); candidate i uses row xrow[i] (xrow NULL: row i);
 *   pos_buf / pos_meta [rows,6] int64: byte offset and length of contig, position and 33-base reference sequence of
 *   a candidate inside pos_buf (what cv_parse_tensor_text emits); candidate i uses row pos_row[i] (NULL: row i);
 *   show_ref: also candidates called REF (--showRef); has_qual / qual_min: --qual (FILTER PASS / LowQual, else ".").
 * Candidates with depth 0 give no record.  Runs on the cv_set_host_threads() threads.
 * Returns 0, or 2 when out_cap is too small (*out_len = bytes needed, nothing written), or 1 (cv_last_error).      */
int cv_format_vcf(const int32_t *call, const float *qual, int64_t n, const float *x, const int64_t *xrow,
                  const char *pos_buf, const int64_t *pos_meta, const int64_t *pos_row, int show_ref,
                  int has_qual, int qual_min, char *out, int64_t out_cap, int64_t *out_len, int64_t *nrecords);
/* The same records written in HBM (csrc/cv_vcf_dev.hip, cv_vcf_core.hpp): the arguments of cv_format_vcf as DEVICE
 * pointers, line i ('\n'-terminated) at text_dev + off_dev[i], dense and in candidate order; off_dev [n + 1] int64,
 * off_dev[n] = bytes in all; info_dev [4] int64 = {bytes, records, CV_VCF_HOST candidates, 0}.  status_dev[i] is
 * CV_VCF_NONE (no record: REF without show_ref, depth 0), CV_VCF_DEVICE (the line is cv_format_vcf's, byte for byte) or
 * CV_VCF_HOST with length 0: what the device does not vouch for and the caller gives to cv_format_vcf, which prints it
 * or refuses it with its own message -- decisions out of range; a quality whose integer is not certain (it is where
 * p2 + 1e-300 == p1 + 1e-300, or where the core's own log puts q further than 2^-40 max(1, |q|) from an integer) or
 * not finite, whatever the depth; a depth that is not a positive integer below 2^24 (0 is CV_VCF_NONE); an allele
 * fraction of 1e9 or more, NaN or infinite; a position that is not 1..18 bare digits; a sequence of 16 bytes or
 * fewer; a contig name above 255 bytes; a centre base outside ACGT where it names the allele.
 * text_dev = NULL: lengths, status and info only.  A line that would end behind text_cap is not written (text_cap =
 * n (longest contig name + 160) holds every batch); nothing behind off_dev[n] is.  call / qual / x 4-byte, the int64
 * arrays 8-byte, the workspace 256-byte aligned.  Asynchronous on `stream`: no allocation, no synchronisation.  n == 0
 * returns 0 and touches nothing; a null or misaligned pointer or n < 0 returns 1.
 * cv_vcf_records_host_form: the same core on the CPU over HOST pointers (tests hold the kernels to it).            */
#define CV_VCF_NONE 0
#define CV_VCF_DEVICE 1
#define CV_VCF_HOST 2
int cv_vcf_records_workspace(int64_t n, int64_t *bytes);
int cv_vcf_records_dev(const int32_t *call_dev, const float *qual_dev, int64_t n, const float *x_dev, const int64_t *xrow_dev,
                       const char *pos_buf_dev, const int64_t *pos_meta_dev, const int64_t *pos_row_dev, int show_ref,
                       int has_qual, int qual_min, int64_t *off_dev, uint8_t *status_dev, int64_t *info_dev, char *text_dev,
                       int64_t text_cap, void *workspace, int64_t workspace_bytes, void *stream);
int cv_vcf_records_host_form(const int32_t *call, const float *qual, int64_t n, const float *x, const int64_t *xrow,
                             const char *pos_buf, const int64_t *pos_meta, const int64_t *pos_row, int show_ref, int has_qual,
                             int qual_min, int64_t *off, uint8_t *status, int64_t *info, char *text, int64_t text_cap);

/* debug / parity: copy one intermediate of the LAST cv_forward chunk to
 * dst_dev in the reference's natural layout ([n,h,4,c] NHWC or [n,units]).
 * layer: 1..3 = pool1..pool3 outputs (for slim: conv outputs), 4 = fc4, 5 = fc5.
 * Serves what getTensorAndLayerPNG.py:30-37 reaches into m.conv1.. for in the slim topology, whose pools are 1;
 * the full topology's maps before pooling come from cv_forward_conv_map.
 * layer 6 / 7 refer to the last cv_grad / cv_loss slice instead: 6 = the alpha-dropout
 * keep mask of fc4 times its affine factor a (selu.py:53-62; 0 where a unit was
 * dropped, a where kept, 1 everywhere at rate 0), 7 = dropout4, the layer's output
 * [n, fc4] -- what the parity tests feed to / compare with the oracle.
 * layer 8 / 9: the same for fc5's alpha-dropout (cv_set_dropout5): 8 = its keep mask times a, 9 = dropout5 [n, fc5];
 * an error after a pass that ran it at rate 0 (cv_loss, or cv_grad with cv_set_dropout5 0).
 * layers 11..13 / 21..23: the pooled maps (slim: conv outputs) and the pre-activation gradients of conv1..conv3 of the
 * last cv_grad / cv_loss pass, natural layout, for its first n candidates -- only when that pass ran as ONE slice
 * (at most 65 536 candidates).  Every other request is an error, never other values: after a pass of several slices
 * (with or without "keep_activations", which extends 6..9 only), for n above the pass's candidates, 21..23 after
 * cv_loss, and 21 of the full topology on the default path (the first layer's unpool rides in its weight-gradient
 * kernel; option dbg4 = 4 materialises it).  tests/test_gpu_train_maps.py holds them to the oracle.
 * Layers 4 / 5 of a pass that ran fc5 and the heads on the tail of the fc4 kernel exist only with option
 * "keep_activations" set before the pass (error otherwise).                        */
int cv_get_activation(cv_model *m, int layer, float *dst_dev, int64_t n, void *stream);

/* debug / parity: the device's SELU (csrc/cv_math.hpp, selu.py:21-25) evaluated on every fp32 bit pattern in
 * [lo_bits, hi_bits] in ascending pattern order; *violations = adjacent pairs, taken as NEGATIVE floats (pattern
 * ascending = value descending), where the output increases; *checksum = wrapping sum of the output bit patterns of
 * all but the first input (the oracle's sweep must give the same).  0x80000000 .. 0xff800000 is the whole negative
 * axis: zero violations there prove SELU monotone, which is what lets the convolution kernels apply max-pooling
 * to the raw accumulators and the activation once per pooled row (max and a monotone map commute).  Synchronous. */
int cv_selu_sweep(int device, uint32_t lo_bits, uint32_t hi_bits, uint64_t *violations, uint64_t *checksum);

/* knobs: "impl" (0 = plain one-thread-per-output kernels, 1 = MFMA tile kernels),
 * "chunk" (candidates per internal pass, 16 .. 2^22, an error beyond; default 65 536; the workspace of a pass takes 41 KB
 * per candidate of the full topology), "profile" (0/1, see cv_kernel_times), "keep_activations" (0/1, default 0:
 * a pass whose fc5 + heads ride on the tail of the fc4 kernel -- variant bit 10 -- also stores the fc4 / fc5 maps,
 * which then only cv_get_activation layers 4 / 5 read; off, those layers report an error after such a pass and the
 * kernel writes a third of the bytes), "train_overlap" (0/1: weight
 * gradients of the training step on a side stream next to the data-gradient chain; default 1, same bits),
 * "infer_small_groups" / "infer_fc4_small_groups" / "infer_slab_groups" (defaults 256 / 288 / -1: cv_forward picks its
 * kernels by the number of groups of 16 candidates in the pass -- up to the first the convolutions unfused with their
 * positions over 8, 4 or 2 waves; up to the second fc4 / fc5 may run as one wave per (group, slab) -- up to
 * "infer_fc4_one_groups" (default 80) fc4 as one wave per (group, output fragment): 1 000 candidates 194 -> 148 us with fc5 + the heads as one launch --; fc4 otherwise as three
 * output slabs on ragged waves (dense_rag) or, with fc5 and the heads on its tail, all 21 tiles per wave: -1 = whichever an
 * estimate of the launch's time says is shorter at this size, >= 0 = the slab form up to that many groups; the same bits
 * whichever runs), "dense_rag" (0 default: the shape of the three-slab fc4 launch -- tile-units per SIMD and workgroup --
 * from the number of groups, so that the time of a pass is proportional to its size; 4..14 = that shape, -1 = the round-5
 * kernel with one group x 7 tiles per wave; A/B and calibration, same bits), "infer_flat" (1 default: the per-group
 * convolution kernel of an inference pass runs on equal ranges of the flat (group, row) sequence when a whole-group launch
 * would leave SIMDs with a wave more than others; 0 = always whole groups, 2 = always flat ranges; same bits),
 * "slim_waves" (0 default: groups per workgroup of the slim topology's conv3 + fc4 kernel -- 8 or 4 -- from the number of
 * groups, so that a small pass spreads over all CUs; 4 / 8 = that many; same bits), "slim_small_groups" (-1 default: a pass
 * of the slim topology runs its layers unfused -- positions split over several waves or equal ranges of the flat (group,
 * row) sequence, fc4 as one wave per (group, output fragment); time linear in the pass -- wherever an estimate says the
 * fused kernels' rounds of workgroups would take longer: a predict() call of 1 000 candidates takes 84 us instead of 400,
 * 32 784 candidates 0.98 ms instead of 1.18; 0..65536 = up to that many groups, fused beyond; same bits),
 * "train_tiny_groups" (0..4096, default 400: training batches of up to that many groups of 16 candidates split the
 * serial loops of their layers over more waves -- same bits; the position parts of the convolutions stop at 80 groups
 * whatever the value), "train_ksplit" (0/1, default 1: at such batches
 * the fc4 forward of the TRAINING pass adds eight partial sums over k ranges instead of one ascending-k chain; fixed
 * order, reproducible run to run, within the gradient tolerance of the single chain, 4 % faster at 1 250 candidates;
 * the slim topology's fc4 -- 396 dependent k steps -- does so at every batch; never used by cv_forward) and
 * "train_side_streams" (1..3, default 3: at such batches the weight gradients of different layers -- independent of
 * each other -- run on up to that many side streams; larger batches use two when the value is >= 2, the second one
 * for the last layers only; same bits),
 * "dbg0".."dbg7" (development A/B switches of the training step, 0 = shipped path; see cv_internal.hpp),
 * "variant" (bit 0: first layer fused into the conv2 kernel, bit 1: MFMA heads kernel,
 * bit 2: 8-wave fc4 workgroups, bit 3: rotating-window conv3 kernel, bit 5: fc4 with two groups of
 * 16 candidates per wave, bit 6: fused conv1+conv2 kernel whose two waves per group share the first layer through
 * LDS (full topology), bit 7: fc4 of passes of up to 256 groups on a kernel without barriers (one wave per group
 * and slab of 3 output fragments, operands prefetched from L2 through a register ring), bit 8: slim topology, conv3
 * and fc4 as one kernel (the conv3 map stays in registers), bit 9: the four heads ride on the fc5 kernel (passes of
 * more than 256 groups whose fc5 is a kernel of its own: 12-16 us of a pass between 5 000 and 50 000 candidates, on by
 * default since round 6), bit 10: fc5 and the four heads on the TAIL
 * of the large-pass fc4 kernel (passes of more than 2 048 groups, full topology: the fc4 output never leaves the
 * registers it was accumulated in; 1.533 -> 1.516 ms for the three layers); default 2031; the alternatives give bit-identical results and exist for A/B
 * timing).                                                                                          */
int cv_set_option(cv_model *m, const char *key, int64_t value);
int cv_get_option(const cv_model *m, const char *key, int64_t *value);

/* Per-kernel device timing of cv_forward (option "profile" = 1): every kernel launch
 * is bracketed by hipEventRecord on the launch stream.  cv_kernel_times synchronises,
 * returns for stage s = 0..CV_NUM_STAGES-1 (conv1, conv2, conv3, fc4, fc5, heads)
 * the summed milliseconds and launch counts since the last call, and resets them.  */
#define CV_NUM_STAGES 6
int cv_kernel_times(cv_model *m, double ms[CV_NUM_STAGES], int64_t launches[CV_NUM_STAGES]);
/* The kernel (template instance as rocprofv3 prints it, without the argument list) stage s of the last cv_forward
 * chunk ran, or NULL if the stage was fused away / the plain kernels ran: lets a measurement taken in another
 * process (rocprofv3 --pmc passes, profiles/pmc_traffic.json) be matched to the binary that is running.          */
int cv_kernel_name(const cv_model *m, int stage, const char **name);

/* ---- training (replaces the session.run calls of train / trainNoRT /
 * getLoss / getLossNoRT, v3.py:183-227, and AdamOptimizer, v3.py:174) ---------- */

/* forward loss with phase False, dropout 0, lambda 0 (getLoss, v3.py:207-216).
 * losses_host[6]: loss1..loss4, lossL2, total -- SUMS over the batch
 * (v3.py:140-151).  Synchronises `stream`.                                      */
int cv_loss(cv_model *m, const float *x_dev, const float *y_dev, int64_t n, double *losses_host,
            void *stream);
/* forward (phase True: alpha-dropout rate `drop4` on fc4, selu.py:34-69; on fc5 the
 * rate of cv_set_dropout5, 0.0 = identity by default) + backward into the flat gradient
 * buffer (data terms only, no lambda term).  seed/step select the counter-based dropout
 * streams (fc5's a domain of its own).
 * losses_host as above with lossL2 = lambda*sum(w^2)/2.  Synchronises.          */
int cv_grad(cv_model *m, const float *x_dev, const float *y_dev, int64_t n, float drop4,
            float lambda, uint64_t seed, uint64_t step, double *losses_host, void *stream);
/* alpha-dropout rate on fc5 (v3.py:121, dropoutRateFC5) of the cv_grad / cv_grad_async passes that follow; never of
 * cv_forward or cv_loss.  [0, 1) is accepted, anything else fails with a message.  Default 0.                   */
int cv_set_dropout5(cv_model *m, float rate);
int cv_get_dropout5(const cv_model *m, float *rate);
/* flat gradient buffer, same order/size as cv_param_buffer (for RCCL all-reduce) */
int cv_grad_buffer(cv_model *m, float **flat_dev, int64_t *count);

/* ---- the optimizer step without host round trips (what train.py's loop and a data-parallel host use) ----
 * The gradient BUCKET is `header` (= 16) floats followed by the flat gradient.  The header carries the losses of
 * the step so that ONE all-reduce(SUM) of the bucket exchanges gradients and losses together: floats 2k, 2k+1 =
 * loss k (base, zygosity, type, length; v3.py:140-148) as a (hi, lo) float pair whose sum is the double the
 * kernels accumulated, floats 8, 9 = lambda * sum(w^2)/2, float 10 = 1 per contributing rank, rest 0.
 * dense_begin = first float of the fc4 / fc5 / head gradients: [dense_begin, count) is 95 % of the bucket and is
 * final early (before the convolution backward pass), [0, dense_begin) at the end of the step.
 * cv_bind_grad_bucket makes the step write into a caller-owned device buffer of `count` floats (16-byte aligned;
 * e.g. a torch tensor that torch.distributed reduces in place -- no staging copies); NULL returns to the
 * library's own.  The caller keeps the buffer alive while it is bound.                                          */
int cv_grad_bucket_info(const cv_model *m, int64_t *count, int64_t *header, int64_t *dense_begin);
int cv_bind_grad_bucket(cv_model *m, float *bucket_dev, int64_t count);
/* cv_grad without the host synchronisation: enqueues forward + backward on `stream` (the weight-gradient kernels
 * on an internal side stream that forks from / joins `stream`; option "train_overlap" = 0 keeps one stream) and
 * the loss header.  comm_stream (may be NULL): made to wait, through an event, for the moment the dense part of
 * the bucket is final, so that an exchange enqueued on it overlaps the rest of the backward pass; the part
 * before dense_begin is final in `stream` order.  The caller orders cv_apply_adam behind its exchange.         */
int cv_grad_async(cv_model *m, const float *x_dev, const float *y_dev, int64_t n, float drop4, float lambda,
                  uint64_t seed, uint64_t step, void *stream, void *comm_stream);
/* add the (exchanged) loss header of the bucket to a device-side accumulator (the L2 term divided by the rank
 * count of float 10) -- train.py only needs the SUM of the batch losses of an epoch (train.py:113-114,123).     */
int cv_loss_accumulate(cv_model *m, void *stream);
/* read the accumulator: losses_host[6] = loss1..loss4, lossL2, total summed over the accumulated steps, *steps =
 * how many (may be NULL); reset != 0 zeroes it.  Synchronises `stream`.                                         */
int cv_loss_read(cv_model *m, double losses_host[6], int64_t *steps, int reset, void *stream);
/* TF1 Adam (beta1 .9, beta2 .999, eps 1e-8, lr_t = lr*sqrt(1-b2^t)/(1-b1^t)) on
 * grad + lambda*w for non-bias variables (l2 term of v3.py:150); t = 1,2,...     */
int cv_apply_adam(cv_model *m, float lr, float lambda, int64_t t, void *stream);
/* cv_apply_adam followed by cv_loss_accumulate in ONE launch (the step of train.run_epoch: a launch less at the tail
 * of every step); same arithmetic as the two calls.                                                            */
int cv_apply_adam_accumulate(cv_model *m, float lr, float lambda, int64_t t, void *stream);
/* optimizer slots m / v (checkpoint variables "<name>/Adam", "<name>/Adam_1")   */
int cv_adam_buffers(cv_model *m, float **m_dev, float **v_dev, int64_t *count);
/* device-to-device copy between a caller buffer (e.g. a torch tensor handed to
 * torch.distributed) and one of the flat buffers: which 0 = parameters,
 * 1 = gradients, 2 = Adam m, 3 = Adam v; to_model != 0 copies caller -> model.  */
int cv_flat_copy(cv_model *m, int which, float *caller_dev, int to_model, void *stream);

/* ---- host data plane (no GPU work) ------------------------------------------------ */

/* Text-tensor reader = the per-row work of utils_v2.GetTensor (utils_v2.py:20-21,33-46;
 * writer dataPrepScripts/CreateTensor.py:24,56).  Parses whole lines
 * "<ctg> <pos> <refSeq33> <528 numbers>" from buf[0,len): rows whose centre base is not
 * A/C/G/T are dropped (utils_v2.py:38-40); x_out[row][528] receives the values with
 * matrices 1..3 minus matrix 0 (utils_v2.py:45-46); meta_out[row][6] = byte offset and
 * length of ctg, pos, seq inside buf.  Stops after max_rows rows or the last complete
 * line; *consumed = bytes eaten, *nrows = rows written, *nbad = malformed rows skipped.  */
int cv_parse_tensor_text(const char *buf, int64_t len, int64_t max_rows, float *x_out,
                         int64_t *meta_out, int64_t *consumed, int64_t *nrows, int64_t *nbad);

/* Host threads cv_parse_tensor_text may use (process-wide, default 1); the rows do not depend on it. */
int cv_set_host_threads(int n);

/* The same reader on the device, for text that is already in HBM: a slab text_dev[0,len) of '\n'-terminated lines at
 * any alignment (the kernels read the 16-byte granules that contain the slab and mask what lies outside it).  Line i
 * of the slab (i < max_lines) gets slot i of every output:
 *   x_dev[max_lines][528] fp32   the row of a line with status ROW (matrices 1..3 minus matrix 0, the bits of
 *                                cv_parse_tensor_text); other slots are not written;
 *   meta_dev[max_lines][6] int64 as cv_parse_tensor_text's, relative to text_dev (ROW slots only);
 *   status_dev[max_lines] uint8  CV_TEXT_ROW; CV_TEXT_SKIP (empty line, sequence of <= 16 bases, centre base not in
 *                                ACGT: dropped silently); CV_TEXT_HOST: the line is not in the producer's format
 *                                (CreateTensor.py:56) -- the device neither accepts nor rejects it, the caller parses
 *                                it with cv_parse_tensor_text;
 *   info_dev[4] int64            bytes consumed (whole lines, at most max_lines of them), lines, ROW lines, HOST lines.
 * The producer's format: "<tok> <tok> <tok>" + 528 x " [-]d{1,9}[.d]", single blanks, no tab / CR / VT / FF anywhere,
 * nothing behind the last value, at most CV_TEXT_LINE_CAP bytes in front of the newline.
 * Everything is enqueued on `stream`; the call neither synchronises nor allocates: `workspace_dev` (256-byte aligned)
 * holds at least cv_parse_tensor_text_dev_workspace(len, max_lines) bytes and belongs to the call until its kernels
 * have run.  x_dev is 16-byte, meta_dev and info_dev are 8-byte aligned.                                             */
#define CV_TEXT_SKIP 0
#define CV_TEXT_ROW 1
#define CV_TEXT_HOST 2
#define CV_TEXT_LINE_CAP 8192
#define CV_TEXT_SLAB_MAX ((int64_t)1 << 31)      /* largest `len` */
int cv_parse_tensor_text_dev_workspace(int64_t len, int64_t max_lines, int64_t *bytes);
int cv_parse_tensor_text_dev(const char *text_dev, int64_t len, int64_t max_lines, float *x_dev, int64_t *meta_dev,
                             uint8_t *status_dev, int64_t *info_dev, void *workspace_dev, int64_t workspace_bytes,
                             void *stream);
/* Compaction behind cv_parse_tensor_text_dev (after the caller has patched the HOST slots): out_dev[r][528] =
 * x_dev[index_dev[r]][528] for r < nrows; index_dev int64 on the device.  Enqueued on `stream`.                       */
int cv_text_gather_rows(const float *x_dev, const int64_t *index_dev, int64_t nrows, float *out_dev, void *stream);
/* What the host still needs of a slab whose text exists only on the device: the three header tokens (contig,
 * position, sequence) of the lines index_dev[0 .. nrows), back to back in bytes_dev[0, bytes_cap), and
 * meta_out_dev[nrows][6] = their offsets / lengths inside bytes_dev -- a (bytes, meta) piece of a position batch after one
 * copy to the host.  meta_dev is cv_parse_tensor_text_dev's (relative to text_dev).  The caller sizes bytes_dev from the
 * token lengths it already holds; a line that would not fit is left out.  Enqueued on `stream`.                       */
int cv_text_gather_tokens(const char *text_dev, const int64_t *meta_dev, const int64_t *index_dev, int64_t nrows,
                          uint8_t *bytes_dev, int64_t bytes_cap, int64_t *meta_out_dev, void *stream);
/* Where lines begin in text that exists only on the device (a reader that owns a byte range of a file several ranks
 * share places the first and the last of its lines with it): for k offsets from[0 .. k) -- a HOST array, k at most
 * CV_TEXT_FIND_MAX -- out_dev[i] = the smallest j >= from[i] with text_dev[j] == '\n', or len when there is none
 * (also when from[i] >= len); a negative offset counts as 0.  text_dev may start at any address: the kernel reads the
 * 16-byte granules that contain text_dev[0, len) and masks what lies outside, as cv_parse_tensor_text_dev does.  One scan
 * serves all k queries (a vector atomic minimum per query and newline; a wave whose text lies behind every answer found
 * so far leaves).  out_dev[k] int64 on the device, 8-byte aligned.  Enqueued on `stream`; neither allocates nor
 * synchronises -- the caller brings out_dev back with whatever else it copies for the slab.                           */
#define CV_TEXT_FIND_MAX 64
int cv_text_find_newline_dev(const char *text_dev, int64_t len, const int64_t *from, int k, int64_t *out_dev, void *stream);

/* BGZF (bgzip / htslib: independent gzip members of <= 64 KiB, the compressed size in the "BC" extra subfield).
 * cv_bgzf_scan walks the member headers of a whole file in memory, once: 0 = BGZF (*members, *inflated_bytes set; the
 * first max_members rows of table[m][4] filled: offset of the DEFLATE data in src, its length, the running output
 * offset, ISIZE << 32 | CRC-32), 1 = not BGZF -- a member without the BC subfield or with other header flags, ISIZE
 * above 65536, a BSIZE that runs past the file, a truncated last member, no member at all; the caller then reads the
 * WHOLE file as ordinary gzip --, -1 = bad arguments.  Zero padding behind the last member, empty members and a file
 * without the EOF marker are accepted.
 * cv_inflate_bgzf_dev inflates `members` rows of such a table on the device: comp_dev points at the first row's DEFLATE
 * data, member i goes to text_dev[out_i - out_0, + ISIZE_i) inside text_dev[0, text_cap) (offsets are taken relative to
 * the first row's).  status_dev[i] = CV_BGZF_OK: a valid stream that produced exactly ISIZE bytes, ended there and has
 * the trailer's CRC-32; CV_BGZF_HOST: anything else -- the device neither accepts nor rejects the member, the caller
 * inflates it with cv_inflate_raw and checks cv_crc32_ieee (its output range may hold anything until then).
 * Enqueued on `stream`; neither allocates nor synchronises.                                                         */
#define CV_BGZF_OK 1
#define CV_BGZF_HOST 2
int cv_bgzf_scan(const uint8_t *src, int64_t n, int64_t max_members, int64_t *table, int64_t *members,
                 int64_t *inflated_bytes);
int cv_inflate_bgzf_dev(const uint8_t *comp_dev, const int64_t *table_dev, int64_t members, uint8_t *text_dev,
                        int64_t text_cap, uint8_t *status_dev, void *stream);

/* Ordinary gzip (one DEFLATE stream, block starts unknown) on the device (csrc/cv_gzip_dev.hip, cv_gzip_core.hpp).
 * All bit offsets count from the first byte of comp_dev / src, least significant bit first.  Everything is enqueued on
 * `stream`; nothing allocates or synchronises.  0 = enqueued, 1 = error (cv_last_error).
 * cv_gzip_header_at (host): 1 when a non-final dynamic-Huffman block header with three complete codes and a code
 *   for symbol 256 stands at `bit` of src[0, n).
 * cv_gzip_chunk_host (host): the decode core's host form over one chunk [start_bit, end_bit) (end_bit < 0: to BFINAL)
 *   -> CV_GZIP_*; *symbols and *ended (the bit it ended at) set; sym (room for cap symbols) may be null to count.
 * cv_gzip_find_dev: found_dev[g] = the first such header in bits [first_bit + g * spacing, first_bit + (g + 1) *
 *   spacing) of comp_dev[0, nbytes) (guess 0 starts one bit later: first_bit itself is the caller's), or -1.
 * cv_gzip_decode_dev: table_dev[c][6] = start bit, end bit (< 0: to BFINAL), offset in sym_dev, symbols to write,
 *   bytes of text that exist in front of the chunk (capped at 32768), 0.  sym_dev null: a counting pass, which reads
 *   the first two and the fifth only.  result_dev[c][4] = symbols, the bit the chunk ended at, CV_GZIP_LANDED (at a
 *   block header exactly at the end bit) / FINAL (the final block ended) / PASSED (went over the end bit) / BAD (not a
 *   stream the core vouches for, input exhausted, more symbols than stated), 0.  A symbol is a byte, or 0x8000 | j =
 *   byte j of the 32 KiB in front of the chunk.  A writing pass never writes outside its [offset, offset + symbols).
 * cv_gzip_resolve_dev: symbols -> text.  off_dev[0 .. chunks] = where each chunk starts (off_dev[chunks] = total), in
 *   sym_dev and in text_dev alike; text_dev[-hist, 0) holds the text in front of the first chunk (hist <= 32768).
 *   *bad_dev is set (never cleared) when a marker reaches in front of the text that exists.
 * cv_gzip_crc_dev: part_dev[p] = the CRC-32 register after the p-th 1 KiB piece of text_dev[0, n), started from 0;
 *   pieces are aligned to the END (the first may be short).                                                        */
#define CV_GZIP_LANDED 1
#define CV_GZIP_FINAL 2
#define CV_GZIP_PASSED 3
#define CV_GZIP_BAD 4
int cv_gzip_header_at(const uint8_t *src, int64_t n, int64_t bit);
int cv_gzip_chunk_host(const uint8_t *src, int64_t n, int64_t start_bit, int64_t end_bit, uint16_t *sym, int64_t cap,
                       int64_t hist, int64_t *symbols, int64_t *ended);
int cv_gzip_find_dev(const uint8_t *comp_dev, int64_t nbytes, int64_t first_bit, int64_t spacing_bytes, int64_t guesses,
                     int64_t *found_dev, void *stream);
int cv_gzip_decode_dev(const uint8_t *comp_dev, int64_t nbytes, const int64_t *table_dev, int64_t chunks, uint16_t *sym_dev,
                       int64_t sym_cap, int64_t *result_dev, void *stream);
int cv_gzip_resolve_dev(const uint16_t *sym_dev, const int64_t *off_dev, int64_t chunks, int64_t total, int64_t hist,
                        uint8_t *text_dev, int32_t *bad_dev, void *stream);
int cv_gzip_crc_dev(const uint8_t *text_dev, int64_t n, uint32_t *part_dev, void *stream);

/* ---- the labelled training set on the device (csrc/cv_trainset.hip) -------------------------------------------------
 * What utils_v2.GetTrainingArray's per-row loop does (utils_v2.py:62-186), for rows cv_parse_tensor_text_dev left in
 * HBM; the host loop stays the definition of the result.  Every call is enqueued on `stream` and neither allocates nor
 * synchronises; workspaces (256-byte aligned) are sized by the *_workspace functions and belong to the call until its
 * kernels have run.
 *
 * cv_trainset_tokens, per slab: row r < nrows is line index_dev[r] of the slab (index_dev null: line r); text_dev /
 * meta_dev as the parser left them.
 *   pos_dev[r] int64, digits_dev[r]  the coordinate token and its length; CV_TRAINSET_BAD_COORD in flags_dev[r] (and
 *                                    digits 0) when it is not canonical decimal: digits only, no leading zero unless it
 *                                    is "0", at most CV_TRAINSET_MAX_DIGITS digits;
 *   centre_dev[r]                    the 17th character of the sequence token, upper-cased: A,C,G,T -> 0..3;
 *   flags_dev[r]                     CV_TRAINSET_RUN_START: the contig token differs byte for byte from row r - 1's (row 0:
 *                                    always); CV_TRAINSET_BAD_SEQ: the sequence token holds ':' or a byte >= 0x80;
 *   run_dev[r] int32                 index of the row's contig run inside the slab (run starts in front of it, minus 1).
 * cv_trainset_join, per slab: run_ctg_dev[nruns] = contig id of each run (the host compares the run-start tokens
 * byte for byte).  Contig ids below `ntab` have rows in the tables: bed_off_dev[ntab + 1] into bed_begin_dev (sorted)
 * / bed_emax_dev (running maximum of the ends), truth_off_dev[ntab + 1] into truth_pos_dev (sorted per contig; null: no
 * truth).  ctg_dev[r] = contig id; keep_dev[r] = !has_bed, or upper_bound(begin, pos) = k > 0 and emax[k - 1] > pos;
 * truth_dev[r] = index of (contig, pos) in truth_pos_dev or -1.
 * cv_trainset_finish, once over all nrows rows in arrival order: the kept rows sorted (stable) by
 * rank_dev[ctg] << 48 | pos * 10^(12 - digits) << 4 | digits -- the order of sorted() over "contig:pos" strings when
 * rank_dev[nctg] orders the contigs by the bytes of name + ":" --, one entry per distinct key:
 *   *total_dev            entries;
 *   src_dev[e] int64      arrival index of the LAST row with the key (buffer of nrows);
 *   y_dev[e][16] fp32     labels_dev[truth][16] when truth >= 0, else HOM, REF, length 0 = 1 and 1 at the centre base
 *                         of the FIRST row with the key (buffer of nrows * 16).
 * cv_trainset_gather: x_out_dev[r][528] = x_all_dev[src_dev[p]][528], y_out_dev[r][16] = y_dev[p][16], p = perm_dev[r]
 * (null: r), r < total; all four tensors 16-byte aligned.                                                            */
#define CV_TRAINSET_RUN_START 1
#define CV_TRAINSET_BAD_COORD 2
#define CV_TRAINSET_BAD_SEQ 4
#define CV_TRAINSET_MAX_DIGITS 12
#define CV_TRAINSET_MAX_CONTIGS 65535
#define CV_TRAINSET_MAX_ROWS ((int64_t)1 << 30)
int cv_trainset_tokens_workspace(int64_t nrows, int64_t *bytes);
int cv_trainset_tokens(const char *text_dev, const int64_t *meta_dev, const int64_t *index_dev, int64_t nrows,
                       int64_t *pos_dev, uint8_t *digits_dev, uint8_t *centre_dev, uint8_t *flags_dev, int32_t *run_dev,
                       void *workspace_dev, int64_t workspace_bytes, void *stream);
int cv_trainset_join(int64_t nrows, const int32_t *run_dev, const int32_t *run_ctg_dev, int64_t nruns,
                     const int64_t *pos_dev, int32_t ntab, int has_bed, const int64_t *bed_off_dev,
                     const int64_t *bed_begin_dev, const int64_t *bed_emax_dev, const int64_t *truth_off_dev,
                     const int64_t *truth_pos_dev, int32_t *ctg_dev, uint8_t *keep_dev, int32_t *truth_dev, void *stream);
int cv_trainset_finish_workspace(int64_t nrows, int64_t *bytes);
int cv_trainset_finish(int64_t nrows, const int32_t *ctg_dev, const int64_t *pos_dev, const uint8_t *digits_dev,
                       const uint8_t *centre_dev, const uint8_t *keep_dev, const int32_t *truth_dev,
                       const int32_t *rank_dev, int32_t nctg, const float *labels_dev, int64_t ntruth, int64_t *src_dev,
                       float *y_dev, int64_t *total_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int cv_trainset_gather(const float *x_all_dev, const float *y_dev, const int64_t *src_dev, const int64_t *perm_dev,
                       int64_t total, float *x_out_dev, float *y_out_dev, void *stream);

/* ---- the truth list and the BED file read on the device (csrc/cv_truth_dev.hip, csrc/cv_truth_core.hpp) ---------------
 * What utils_v2._read_bed_truth + utils_v2._trainset_tables do per line of the two small text inputs of the training-set
 * builders (utils_v2.truth_tables); the host loop stays the definition.  Every *_dev call is enqueued on `stream` and
 * neither allocates nor synchronises; workspaces (256-byte aligned) are sized by the *_workspace functions and belong to
 * the call until its kernels have run.
 *
 * cv_truth_lines_dev, per slab of text: the lines that END inside text_dev[0, len) (at most max_lines of them), each given
 * one verdict -- a ROW with its fields, a line the definition SKIPs (no token), or a line only the definition can answer
 * (HOST: a byte outside 0x21..0x7E / space / tab, more than CV_TRUTH_LINE_CAP bytes, too few tokens, an integer that is
 * not canonical decimal of at most CV_TRAINSET_MAX_DIGITS digits, a ':' in the contig token, a first base outside ACGT
 * where utils_v2._label looks it up).  Format VAR is "ctg pos ref alt g1 g2", BED "ctg begin end".  Format VCF is a line
 * of a truth VCF under GetTruth's rules for ONE source -- ctg[ctg_len] (a HOST pointer, 1 .. CV_TRUTH_MAX_CTG bytes) the
 * wanted contig, [lower, upper] its bounds when has_bounds; the four arguments are ignored for the other formats --: a
 * line whose first token starts with '#' or is another contig, or whose position lies outside the bounds, is SKIPped
 * whatever else it holds; the genotype (last column up to ':') must be digit-or-'.', '/' or '|', digit-or-'.', else HOST;
 * p1 <= p2; 1|2 with a ',' in ALT becomes 0|1 on the first of the shortest ALT alleles; the row's fields are those of
 * "ctg pos REF ALT p1 p2" in format VAR.  The per-line status stays in the workspace: the outputs are the rows and the
 * counters, which is what a whole-call hand-over needs.  Row r = the r-th ROW:
 *   pos_dev[r] int64      VAR: pos; BED: begin;
 *   end_dev[r] int64      BED only: int(end) - 1, + 1 when that equals begin (may be null for VAR);
 *   label_dev[r][16] fp32 VAR and VCF: utils_v2._label of the row (may be null for BED);
 *   run_dev[r] int32      index of the row's contig run: a run starts at a ROW whose contig token differs byte for byte
 *                         from the line before, or whose line before is no ROW;
 *   tok_dev[k][2] int64   offset in the slab and length of the contig token that starts run k;
 *   info_dev[8] int64     {bytes consumed, lines, rows, skipped, host, runs, 0, 0}.
 * The four row arrays hold max_lines entries.  cv_truth_lines_host_form: the same core on the CPU over HOST pointers.
 *
 * cv_bed_table_dev, once over the n intervals of all slabs, run_ctg_dev[nruns] = contig id of each run (the host compares
 * the run-start tokens): the intervals of each contig sorted by (begin, end); bed_off_dev[nctg + 1], bed_begin_dev[n],
 * bed_emax_dev[n] = running maximum of the ends within the contig -- the tables cv_trainset_join reads.  In both table
 * calls a run index outside [0, nruns) or a contig id outside [0, nctg) is the caller's error and counts as contig 0.
 *
 * cv_truth_tables_dev, once over the n truth rows of all slabs in arrival order: the last row of each (contig id, pos)
 * wins; those the BED keeps (has_bed: upper_bound(begin, pos) = k > 0 and emax[k - 1] > pos; else all) give
 * truth_off_dev[nctg + 1], truth_pos_dev (ascending per contig), labels_dev[..][16]; all of them give every_off_dev
 * [nctg + 1], every_pos_dev: the distinct positions per contig.  counts_dev[2] = {truth rows, distinct positions}; the
 * three row arrays hold n entries; label_dev / labels_dev 16-byte aligned.                                             */
#define CV_TRUTH_FORMAT_VAR 0
#define CV_TRUTH_FORMAT_BED 1
#define CV_TRUTH_FORMAT_VCF 2
#define CV_TRUTH_MAX_CTG 256
#define CV_TRUTH_LINE_CAP 8192
#define CV_TRUTH_MAX_LINES ((int64_t)1 << 27)
int cv_truth_lines_workspace(int64_t len, int64_t max_lines, int64_t *bytes);
int cv_truth_lines_dev(const char *text_dev, int64_t len, int format, const char *ctg, int64_t ctg_len, int has_bounds,
                       int64_t lower, int64_t upper, int64_t max_lines, int64_t *pos_dev, int64_t *end_dev, float *label_dev,
                       int32_t *run_dev, int64_t *tok_dev, int64_t *info_dev, void *workspace_dev, int64_t workspace_bytes,
                       void *stream);
int cv_truth_lines_host_form(const char *text, int64_t len, int format, const char *ctg, int64_t ctg_len, int has_bounds,
                             int64_t lower, int64_t upper, int64_t max_lines, int64_t *pos, int64_t *end, float *label,
                             int32_t *run, int64_t *tok, int64_t *info);
int cv_bed_table_workspace(int64_t n, int64_t *bytes);
int cv_bed_table_dev(int64_t n, const int64_t *begin_dev, const int64_t *end_dev, const int32_t *run_dev,
                     const int32_t *run_ctg_dev, int64_t nruns, int32_t nctg, int64_t *bed_off_dev, int64_t *bed_begin_dev,
                     int64_t *bed_emax_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int cv_truth_tables_workspace(int64_t n, int64_t *bytes);
int cv_truth_tables_dev(int64_t n, const int64_t *pos_dev, const float *label_dev, const int32_t *run_dev,
                        const int32_t *run_ctg_dev, int64_t nruns, int32_t nctg, int has_bed, const int64_t *bed_off_dev,
                        const int64_t *bed_begin_dev, const int64_t *bed_emax_dev, int64_t *truth_off_dev,
                        int64_t *truth_pos_dev, float *labels_dev, int64_t *every_off_dev, int64_t *every_pos_dev,
                        int64_t *counts_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- the dataPrepScripts helpers on the device (csrc/cv_beditems_dev.hip, csrc/cv_beditems_core.hpp) ------------------
 * ChooseItemInBed / CountNumInBed keep the LINES of a file whose first two columns are contig and position when a BED
 * interval covers the position; RandomSampling keeps the POSITIONS of a range that a BED covers and a keyed draw selects.
 * The host loops of clairvoyante_amd/bed_items.py stay the definitions.  As above, every *_dev call is enqueued on
 * `stream` and neither allocates nor synchronises; workspaces (256-byte aligned) are sized by the *_workspace functions.
 *
 * cv_item_lines_dev, per slab of item text: the lines that END inside text_dev[0, len) (at most max_lines), each given a
 * verdict by csrc/cv_truth_core.hpp in format CV_TRUTH_FORMAT_ITEM -- a ROW (two tokens, the second canonical decimal of
 * at most CV_TRAINSET_MAX_DIGITS digits; what follows is held to the byte rule only) or HOST (a blank line, one token,
 * "007", "+5", '\r', a byte outside 0x21..0x7E / space / tab, more than CV_TRUTH_LINE_CAP bytes).  There is no SKIP.
 * Row r = the r-th ROW:
 *   pos_dev[r] int64      the position;
 *   run_dev[r] int32      index of the row's contig run (as in cv_truth_lines_dev);
 *   off_dev[r] int64      offset of the line's first byte in the slab;
 *   len_dev[r] int64      its length, the newline included;
 *   tok_dev[k][2] int64   offset in the slab and length of the contig token that starts run k;
 *   info_dev[8] int64     {bytes consumed, lines, rows, 0, host, runs, 0, 0}.
 * The row arrays hold max_lines entries.  cv_item_lines_host_form: the same core on the CPU over HOST pointers.
 *
 * cv_items_keep_dev, over the n rows of one slab: run_ctg_dev[nruns] = the BED contig id of each run, -1 for a contig the
 * BED lacks (the host compares the run-start tokens; the rows may be a part of the slab's rows, so nruns may exceed n);
 * bed_off / bed_begin / bed_emax are cv_bed_table_dev's tables over nctg contigs.  A row is kept when its id is not -1 and upper_bound(begin, pos) = k > 0 and emax[k - 1] > pos.  With
 * want_text the kept lines' bytes go to out_text_dev[0, out_cap) in order, one behind the other (an exclusive sum of their
 * lengths places them; one wave copies one line, in 16-byte granules where source and destination agree modulo 16); a
 * line that would not fit, or that does not lie inside the slab, is not copied.  counts_dev[4] = {rows, kept rows, kept
 * bytes, 0}; without want_text neither the sum nor the copy runs and kept bytes is 0.
 * cv_items_keep_host_form: the same on the CPU, the copy lane by lane.
 *
 * cv_items_copy_dev, over n lines of one slab whose verdicts the caller has already (PairWithNonVariants' device route:
 * the pairing decides over the rows of whole files, the gather runs per slab): cv_items_keep_dev's gather without its
 * BED test.  off_dev[n] = offset of each line's first byte in text_dev[0, len), kept_len_dev[n] = its length when it is
 * kept, 0 when it is not.  The kept lines' bytes go to out_text_dev[0, out_cap) in order, one behind the other: the
 * lengths are copied into the workspace, an exclusive sum places them, and the SAME copy kernel moves them (one wave per
 * line).  A line that does not lie inside the text, or would not fit the room, is not copied, and a negative length is
 * the caller's error and never copied: nothing outside either buffer is touched.  counts_dev[4] = {0, 0, sum of the
 * lengths, 0} (the layout of cv_items_keep_dev's counters; the caller knows its rows).  Asynchronous on `stream`, the
 * workspace (cv_items_copy_workspace(n)) is the caller's and belongs to the call until its launches have run.
 * cv_items_copy_host_form: the same bytes and counters from the same core on the CPU.
 *
 * cv_sample_positions_dev, one tile of positions first .. first + count - 1 of the contig whose name hashes to h
 * (FNV-1a-32): a position is kept when the contig's sorted table bed_begin_dev / bed_emax_dev[nbed] covers it (nbed = 0:
 * no BED, every position passes) and cv_draw(seed, 2, h, pos, 0) <= prob in double.  The kept positions go to
 * out_pos_dev[0, cap) ascending; count_dev[2] = {positions written, positions kept}: where they differ `cap` was too
 * small and the caller repeats the tile.  The workspace depends on count (at most CV_SAMPLE_MAX_TILE) alone.          */
#define CV_TRUTH_FORMAT_ITEM 3
#define CV_SAMPLE_MAX_TILE ((int64_t)1 << 28)
int cv_item_lines_workspace(int64_t len, int64_t max_lines, int64_t *bytes);
int cv_item_lines_dev(const char *text_dev, int64_t len, int64_t max_lines, int64_t *pos_dev, int32_t *run_dev, int64_t *off_dev,
                      int64_t *len_dev, int64_t *tok_dev, int64_t *info_dev, void *workspace_dev, int64_t workspace_bytes,
                      void *stream);
int cv_item_lines_host_form(const char *text, int64_t len, int64_t max_lines, int64_t *pos, int32_t *run, int64_t *off,
                            int64_t *llen, int64_t *tok, int64_t *info);
int cv_items_keep_workspace(int64_t n, int64_t *bytes);
int cv_items_keep_dev(const char *text_dev, int64_t len, int64_t n, const int64_t *pos_dev, const int32_t *run_dev,
                      const int64_t *off_dev, const int64_t *len_dev, const int32_t *run_ctg_dev, int64_t nruns, int32_t nctg,
                      const int64_t *bed_off_dev, const int64_t *bed_begin_dev, const int64_t *bed_emax_dev, int want_text,
                      char *out_text_dev, int64_t out_cap, int64_t *counts_dev, void *workspace_dev, int64_t workspace_bytes,
                      void *stream);
int cv_items_keep_host_form(const char *text, int64_t len, int64_t n, const int64_t *pos, const int32_t *run, const int64_t *off,
                            const int64_t *llen, const int32_t *run_ctg, int64_t nruns, int32_t nctg, const int64_t *bed_off,
                            const int64_t *bed_begin, const int64_t *bed_emax, int want_text, char *out_text, int64_t out_cap,
                            int64_t *counts);
int cv_items_copy_workspace(int64_t n, int64_t *bytes);
int cv_items_copy_dev(const char *text_dev, int64_t len, int64_t n, const int64_t *off_dev, const int64_t *kept_len_dev,
                      char *out_text_dev, int64_t out_cap, int64_t *counts_dev, void *workspace_dev, int64_t workspace_bytes,
                      void *stream);
int cv_items_copy_host_form(const char *text, int64_t len, int64_t n, const int64_t *off, const int64_t *kept_len,
                            char *out_text, int64_t out_cap, int64_t *counts);
int cv_sample_positions_workspace(int64_t count, int64_t *bytes);
int cv_sample_positions_dev(uint64_t seed, uint32_t h, int64_t first, int64_t count, double prob, int64_t nbed,
                            const int64_t *bed_begin_dev, const int64_t *bed_emax_dev, int64_t *out_pos_dev, int64_t cap,
                            int64_t *count_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* c-blosc 1.x chunk codec for the 500-item blocks of the `.bin` training file
 * (utils_v2.py:159-186 blosc.pack_array(cname='lz4hc'), :189-207 blosc.unpack_array;
 * tensor2Bin.py:24-28).  Decoder: LZ4/LZ4HC streams, byte shuffle, split blocks, memcpy'd
 * chunks.  Encoder: one LZ4 block with byte shuffle (readable by c-blosc).              */
int64_t cv_blosc_nbytes(const uint8_t *chunk, int64_t clen);
int cv_blosc_decompress(const uint8_t *chunk, int64_t clen, uint8_t *dst, int64_t dstcap);
int cv_blosc_compress_lz4(const uint8_t *src, int64_t n, int typesize, uint8_t *dst, int64_t dstcap,
                          int64_t *clen);
/* n chunks at once on the host threads of cv_set_host_threads (the blocks of one DecompressArray call,
 * utils_v2.py:196-203); status[i] != 0 marks a chunk that failed.                                  */
int cv_blosc_decompress_many(const uint8_t *const *chunks, const int64_t *clens, uint8_t *const *dsts,
                             const int64_t *dstcaps, int64_t n, int32_t *status);
/* The same blocks straight into ONE array: each chunk holds one pickled ndarray (blosc.pack_array); its raw data is
 * located inside the decompressed pickle and copied to dst + i*block_bytes (every block but the last must hold
 * exactly block_bytes).  lens[i] = data bytes of block i; status[i] = 0 ok / 1 corrupt / 2 layout not recognised (the
 * caller then un-pickles instead).  Returns 0 only if all blocks are ok.                                */
int cv_blosc_unpack_blocks(const uint8_t *const *chunks, const int64_t *clens, int64_t n, uint8_t *dst,
                           int64_t block_bytes, int64_t *lens, int32_t *status);
/* A second writer: c-blosc's own multi-block layout.  The data is cut into blocks of `blocksize` bytes (rounded down
 * to whole elements and to the data, as c-blosc does; 1 <= typesize <= 16); every block is byte-shuffled on its own and, when blocksize / typesize >= 128 and the
 * block is not the leftover, split into `typesize` byte-plane LZ4 streams (the rule cv_blosc_decompress reads); a
 * split whose LZ4 form is not smaller is stored.  Chunks of fewer than 64 bytes, and chunks that do not shrink, are
 * memcpy'd.  dstcap >= cv_blosc_blocks_bound(n, typesize, blocksize).  cv_blosc_compress_lz4 stays the default writer. */
int64_t cv_blosc_blocks_bound(int64_t n, int typesize, int64_t blocksize);
int cv_blosc_compress_lz4_blocks(const uint8_t *src, int64_t n, int typesize, int64_t blocksize, uint8_t *dst,
                                 int64_t dstcap, int64_t *clen);

/* The same blocks decoded on the device (csrc/cv_blosc_dev.hip): the compressed chunks cross to HBM, not 2 112 bytes
 * per candidate.  None of the three allocates or synchronises; the two *_dev calls are enqueued on `stream`.
 * cv_blosc_plan (host, no GPU) reads the 16-byte header, bstarts and per-split length words of n chunks with the checks
 * of cv_blosc_decompress and lays the chunks out back to back (16-byte aligned) in a slab of *comp_bytes and their
 * byte planes in a scratch of *scratch_bytes.  It writes
 *   stream_rows[CV_BLOSC_STREAM_ROW * s]: offset of the stream in the slab, cb, offset in the scratch, neblock,
 *                                         1 = stored (cb == neblock, a plain copy; a memcpy'd chunk is one such row)
 *   chunk_rows[CV_BLOSC_CHUNK_ROW * i]:   typesize, shuffle flag, nbytes, blocksize, first stream, stream count,
 *                                         scratch offset, 1 = not for the device, offset of the chunk in the slab, clen
 * A chunk is "not for the device" when the host decoder would refuse it (version != 2, truncated tables, bad offsets),
 * when it is not byte-shuffled LZ4 (bit shuffle, another codec), when typesize is not 1, 4 or 8, when nbytes >
 * max_nbytes or when max_streams rows do not hold it; it takes no room in the slab.  Returns the number of such chunks
 * (0 = all planned), -1 on a bad argument.
 * cv_blosc_decode_dev decodes `streams` rows, one wave per row, from the slab into the scratch; status_dev[s] =
 * CV_BLOSC_OK: the stream consumed exactly cb bytes and produced exactly neblock; CV_BLOSC_HOST: anything else -- the
 * device neither accepts nor rejects it, the host decoder has the last word.  Rows that do not lie inside
 * [0, comp_bytes) / [0, scratch_bytes) are not touched (HOST).
 * cv_blosc_unpack_dev unshuffles each chunk's planes (per blosc block; the leftover block has its own element count),
 * finds the pickled ndarray's data in the first 1 KiB by the rule of cv_blosc_unpack_blocks and writes it to
 * dst_dev + i * block_bytes.  lens_dev[i] = data bytes of chunk i; status_dev[i] as cv_blosc_unpack_blocks: 0 ok, 1 a
 * stream came back HOST or the chunk was not planned, 2 payload not recognised or of unexpected size (not block_bytes
 * for a chunk that is not the last, more than block_bytes); a last chunk of fewer than 512 bytes without a payload
 * (the always-appended empty block) is ok with length 0.  At most 65535 chunks per call.                          */
#define CV_BLOSC_OK 1
#define CV_BLOSC_HOST 2
#define CV_BLOSC_STREAM_ROW 5
#define CV_BLOSC_CHUNK_ROW 10
int cv_blosc_plan(const uint8_t *const *chunks, const int64_t *clens, int64_t n, int64_t max_nbytes, int64_t max_streams,
                  int64_t *stream_rows, int64_t *chunk_rows, int64_t *streams, int64_t *comp_bytes, int64_t *scratch_bytes);
int cv_blosc_decode_dev(const uint8_t *comp_dev, int64_t comp_bytes, const int64_t *stream_rows_dev, int64_t streams,
                        uint8_t *scratch_dev, int64_t scratch_bytes, uint8_t *status_dev, void *stream);
int cv_blosc_unpack_dev(const int64_t *chunk_rows_dev, int64_t chunks, const uint8_t *stream_status_dev, int64_t streams,
                        const uint8_t *scratch_dev, int64_t scratch_bytes, uint8_t *dst_dev, int64_t block_bytes,
                        int64_t *lens_dev, int32_t *status_dev, void *stream);

/* The X blocks of a resident training set packed on the device (csrc/cv_blosc_pack_dev.hip; the encode core is
 * csrc/cv_lz4enc_core.hpp).  A chunk is head | data_bytes_per_chunk bytes of rows | tail -- the pickle envelope of
 * blosc.pack_array around the rows where they lie in HBM -- and is written in the layout of cv_blosc_compress_lz4_blocks
 * (byte shuffle; blocks of `blocksize` bytes split into byte planes; one LZ4 block per plane, one wave each; a plane
 * that does not shrink is stored).  All chunks of a call share one envelope (at most 2 048 bytes each of head and tail,
 * host memory, copied once), so a partial last chunk is a call of its own.  Only typesize 4 is taken, and only chunks of
 * at least 64 bytes whose streams hold at most cv_blosc_pack_stream_cap() bytes: anything else is an error, and the
 * caller packs on the host.
 * cv_blosc_pack_workspace -> the bytes of workspace_dev (16-byte aligned) and of out_dev a call over `chunks` (at most
 * 65535) chunks of chunk_nbytes = head_len + data_bytes_per_chunk + tail_len bytes needs.
 * cv_blosc_pack_dev enqueues the three phases on `stream`, allocates nothing and does not synchronise:
 *   status_dev[c]    CV_BLOSC_OK: chunk c lies at out_dev[chunk_off_dev[c], chunk_off_dev[c + 1]);  CV_BLOSC_HOST: it
 *                    would not be smaller than 16 + nbytes (the host writer memcpy's such a chunk) -- it takes no room,
 *                    the caller packs it with cv_blosc_compress_lz4_blocks
 *   chunk_off_dev    int64[chunks + 1], 8-byte aligned; only out_dev[0, chunk_off_dev[chunks]) needs to cross
 * cv_blosc_pack_phase_dev launches one phase alone (0 encode, 1 layout, 2 assemble) on buffers a whole call has filled:
 * for the probe's timing.
 * cv_blosc_pack_host_form writes the same chunks with the host form of the core, from host memory into host memory
 * (out_cap as cv_blosc_pack_workspace says): byte for byte what the device writes.                                    */
int64_t cv_blosc_pack_stream_cap(void);
int cv_blosc_pack_workspace(int64_t chunks, int64_t chunk_nbytes, int typesize, int64_t blocksize, int64_t *scratch_bytes,
                            int64_t *out_bound);
int cv_blosc_pack_dev(const uint8_t *data_dev, int64_t chunks, int64_t data_bytes_per_chunk, const uint8_t *head, int64_t head_len,
                      const uint8_t *tail, int64_t tail_len, int typesize, int64_t blocksize, uint8_t *out_dev, int64_t out_cap,
                      int64_t *chunk_off_dev, int32_t *status_dev, uint8_t *workspace_dev, int64_t workspace_bytes, void *stream);
int cv_blosc_pack_phase_dev(int phase, const uint8_t *data_dev, int64_t chunks, int64_t data_bytes_per_chunk, int64_t head_len,
                            int64_t tail_len, int typesize, int64_t blocksize, uint8_t *out_dev, int64_t out_cap,
                            int64_t *chunk_off_dev, int32_t *status_dev, uint8_t *workspace_dev, int64_t workspace_bytes, void *stream);
int cv_blosc_pack_host_form(const uint8_t *data, int64_t chunks, int64_t data_bytes_per_chunk, const uint8_t *head, int64_t head_len,
                            const uint8_t *tail, int64_t tail_len, int typesize, int64_t blocksize, uint8_t *out, int64_t out_cap,
                            int64_t *chunk_off, int32_t *status);

/* CRC32C (Castagnoli) of the tensor bytes / table blocks of the TensorFlow V2 checkpoint
 * bundle written by saveParameters and read by restoreParameters (v3.py:243-251).        */
uint32_t cv_crc32c(uint32_t crc, const void *data, int64_t n);

/* ---- pileup front end: alignments -> count tensors -------------------------
 * Replaces the body of dataPrepScripts/CreateTensor.py: the per-read CIGAR walk of
 * OutputAlnTensor (:140-246) and the per-candidate accumulation of GenerateTensor (:23-54).
 * The host parses SAM text (what `samtools view -F 2308` prints, :128-130) into alignment
 * segments; a scatter kernel adds every alignment column to the counters of the candidates whose
 * 33-position window holds it; a finalize kernel writes the [n,33,4,4] tensors in HBM, either raw
 * (what CreateTensor.py prints with "%0.1f", :52) or already with matrices 1..3 minus matrix 0
 * (what utils_v2.GetTensor hands to the network, utils_v2.py:46) so they can feed cv_forward
 * without the text round trip.  Not modelled: the reference's 10 000 000-column buffering cap
 * (`availableSlots`, :96) which silently drops columns in extremely deep regions.             */
typedef struct cv_pileup cv_pileup;

/* min_mq: --minMQ (:153); dcov: --dcov, reads beyond that many sharing one POS are skipped
 * (:165-172); consider_left_edge: --considerleftedge (:63-71).                                 */
int cv_pileup_create(int device, int min_mq, int dcov, int consider_left_edge, cv_pileup **out);
void cv_pileup_destroy(cv_pileup *p);

/* Reference bases as `samtools faidx` printed them (case and N kept: only upper-case ACGT count,
 * :28-31).  seq[0] is the 0-based contig position `first_pos0` (refStart-1, :99-104).  Copied.  */
int cv_pileup_set_reference(cv_pileup *p, const char *seq, int64_t len, int64_t first_pos0);

/* Candidate centres: 1-based positions, strictly ascending (GetCandidate :56-62 after its contig /
 * range filter).  Allocates and zeroes the device counters.  Copied.                           */
int cv_pileup_set_candidates(cv_pileup *p, const int64_t *centers, int64_t n);

/* Parse whole SAM lines from text[0..nbytes); *consumed = bytes up to the last complete line (feed
 * the rest again with the next chunk; pass final != 0 to take an unterminated last line too).
 * Header lines, reads below min_mq and reads beyond dcov are dropped exactly like :146-172; the
 * POS / depth-cap state carries over between calls.  *kept = reads queued by this call.          */
int cv_pileup_add_sam(cv_pileup *p, const char *text, int64_t nbytes, int final, int64_t *consumed,
                      int64_t *kept);

/* The same reads straight from BAM records (cv_bam_view_records): every record is taken as the line
 * `samtools view` prints for it (SEQ "*" for an absent sequence, no CIGAR operations for "*"; the RNAME test
 * of the candidate pass is the flag contig_ok: the view's contig is the one of cv_pileup_set_contig).
 * Same filters, same running state, same result as cv_pileup_add_sam on that text.                 */
int cv_pileup_add_bam(cv_pileup *p, const uint8_t *base, const uint32_t *offs, int64_t n, int contig_ok,
                      int64_t *kept);

/* Bases queued on the host and not yet scattered (callers flush when this gets large).          */
int64_t cv_pileup_pending(const cv_pileup *p);

/* Upload the queued segments and run the scatter kernel on `stream`; returns after the launch.   */
int cv_pileup_flush(cv_pileup *p, void *stream);

/* Flush, then write per candidate i: tensors_dev[i] = [33,4,4] fp32 counts (subtract != 0: matrices
 * 1..3 minus matrix 0), depth_dev[i] = aligned depth at the centre column (the --minCoverage test,
 * :51), touched_dev[i] = 1 iff some read was activated for it (only those get a row, :232-246).
 * Any output pointer may be NULL.  Counters stay valid: more reads may be added afterwards.     */
int cv_pileup_finish(cv_pileup *p, float *tensors_dev, int32_t *depth_dev, uint8_t *touched_dev,
                     int subtract, void *stream);

/* HIP-event time of the launches since creation: ms[0] scatter total, ms[1] finalize total, ms[2]
 * candidate pass (count + select); counts[0] alignment columns queued, counts[1] segments,
 * counts[2] scatter launches.                                                                   */
int cv_pileup_stats(cv_pileup *p, float ms[3], int64_t counts[3]);

/* ---- candidate extraction on the same alignments ------------------------------------------------
 * Replaces the body of dataPrepScripts/ExtractVariantCandidates.py (MakeCandidates :118-246,
 * OutputCandidate :22-42).  Options (before the first read): "evc" = 1 also books every read that
 * passes the candidate filters (contig, "evc_min_mq", >= 55 % aligned, :137-160) into per-position
 * counters A,C,G,T,I,D,N over the reference window; "retain" = 1 keeps the uploaded alignments in
 * HBM so that cv_pileup_adopt_candidates can run the tensor scatter over them again -- the SAM text
 * is parsed once for both steps (the reference pipes `samtools view` twice, callVarBam.py:116-131).
 * "threads" = host threads cv_pileup_add_sam may use on chunks of >= 1 MiB (the result does not depend
 * on it: records are parsed independently, the POS-run state is applied afterwards in read order).   */
int cv_pileup_set_option(cv_pileup *p, const char *key, int64_t value);
int cv_pileup_set_contig(cv_pileup *p, const char *name);        /* RNAME test of the candidate pass */

/* Flush, then select the positions OutputCandidate would print: total count >= min_coverage and
 * (top fraction <= 1 - threshold and second fraction >= threshold, or top symbol != reference base);
 * has_region: 0-based position in [ctg_start, ctg_end] as the reference compares them (:181-183, i.e.
 * ctg_start already +1); nbed >= 0: position inside one of the half-open BED intervals (:90-103), -1 =
 * no BED file.  Ties keep the order A,C,G,T,I,D,N (insertion order; see tests/golden/make_golden_evc.py).
 * *n_out = entries selected (a position may have a second, "late" entry, :215-241).               */
int cv_pileup_extract_candidates(cv_pileup *p, double threshold, double min_coverage, int has_region,
                                 int64_t ctg_start, int64_t ctg_end, const int64_t *bed_begin,
                                 const int64_t *bed_end, int64_t nbed, void *stream, int64_t *n_out);

/* The selected entries (host arrays of n_out elements; any may be NULL): 0-based position, 1 for a
 * late entry, the seven counts in A,C,G,T,I,D,N order; info[0] = reads the pass took (processedReads,
 * :150), info[1] = 0-based POS of the last of them (positions from there on are reported by the
 * reference's final loop, :215-241, together with the late entries).                            */
int cv_pileup_get_extracted(cv_pileup *p, int64_t *pos0, int32_t *late, int32_t *counts7, int64_t info[2]);

/* Make the selected positions (+1, optionally restricted to [lo1, hi1] like CreateTensor.py:60-61)
 * the candidate centres and scatter the retained alignments into their counters.               */
int cv_pileup_adopt_candidates(cv_pileup *p, int has_range, int64_t lo1, int64_t hi1, void *stream,
                               int64_t *n_out);

/* Zero the per-position counters and run the candidate-pass count kernel again over the retained
 * alignments (measurement: repeats the device pass without re-parsing; same result).            */
int cv_pileup_recount(cv_pileup *p, void *stream);

/* Current candidate centres (1-based); centers may be NULL to query the count.                  */
int cv_pileup_get_candidates(cv_pileup *p, int64_t *centers, int64_t cap, int64_t *n_out);

/* ---- the labelled training set straight from the pileup (csrc/cv_bamtrain.hip, csrc/cv_draw_core.hpp) ----------
 * Replaces the middle of dataPrepScripts/PrepDataBeforeDemo.sh -- ExtractVariantCandidates.py --gen4Training, the two
 * CreateTensor.py runs and PairWithNonVariants.py -- for utils_v2.GetTrainingSetFromBam; what follows them is the
 * cv_trainset_* block above.  The reference draws from Python's unseeded generator in file order; here a draw is
 * Philox4x32-10 keyed by what is drawn: key = the halves of `seed`, counter = (pos lo32, pos hi32, stream | late << 8,
 * h), pos the 1-based coordinate, h = FNV-1a-32 of the contig name, stream CV_DRAW_SAMPLE (0) or CV_DRAW_PAIR (1);
 * u = ((x0 << 32 | x1) >> 11) * 2^-53.
 *
 * cv_draws_host (host, no GPU): out_u[i] = that draw for (pos[i], late[i]); late may be NULL (all 0).
 *
 * cv_pileup_sample_candidates: cv_pileup_extract_candidates with threshold 0 and min_coverage 0 (every position the
 *   "evc" pass booked, inside the region and the BED; a late second entry is its own entry) of which an entry stays
 *   unless its stream-0 draw u > output_prob (:203).  Needs cv_pileup_set_contig (the name keys the draws).  The entries
 *   stay in HBM, only *n_out comes back; cv_pileup_get_extracted fetches them when asked.
 * cv_pileup_adopt_union (needs "retain"): centres = the sorted, unique union of the sampled positions (+1, inside
 *   [lo1, hi1] when has_range) and truth[ntruth] (host, strictly ascending 1-based positions: the truth rows of the
 *   contig the caller found inside the range, CreateTensor.py:59-61), with CV_CENTRE_TRUTH / CV_CENTRE_SAMPLED per
 *   centre; then the scatter over the retained alignments as cv_pileup_adopt_candidates runs it.
 * cv_bamtrain_columns, behind cv_pileup_finish(depth_dev, touched_dev), per centre i < n:
 *   row_dev[i]     CreateTensor.py prints a row (:50-51): touched, the window starts inside the loaded reference,
 *                  depth >= min_coverage
 *   pos_dev[i] int64, digits_dev[i]  the centre and its decimal length (0 for a centre <= 0)
 *   centre_dev[i]  the upper-cased reference base at the centre -> 0..3 (255: none of A, C, G, T), acgt_dev[i] = it is one
 *   flags_dev[i]   the centre's CV_CENTRE_* flags
 * cv_bamtrain_pair, once over the nrows rows of ALL sources (PairWithNonVariants.py pairs the concatenated files):
 *   keep_dev[r] holds the BED verdict of cv_trainset_join on entry.  v = rows with CV_CENTRE_TRUTH (not BED-filtered,
 *   :50-62), c = the other rows the BED keeps (:68-86), r = min(1, amp * v / c) in double, r = 1 when c == 0 (the
 *   reference divides by zero); keep_dev[r] = truth ? BED verdict : (BED verdict and stream-1 draw of (ctg_hash_dev[
 *   ctg_dev[r]], pos_dev[r]) < r), AND acgt_dev[r] -- a row whose centre is not ACGT is dropped only by the reader
 *   behind the pairing, so it still counts in c.  counts_dev[4] = v, c, non-variants picked (before acgt), rows kept;
 *   *r_dev = r: all the host fetches.                                                                              */
#define CV_CENTRE_TRUTH 1
#define CV_CENTRE_SAMPLED 2
int cv_draws_host(uint64_t seed, int stream, uint32_t h, const int64_t *pos, const int32_t *late, int64_t n, double *out_u);
int cv_pileup_sample_candidates(cv_pileup *p, uint64_t seed, double output_prob, int has_region, int64_t ctg_start,
                                int64_t ctg_end, const int64_t *bed_begin, const int64_t *bed_end, int64_t nbed,
                                void *stream, int64_t *n_out);
int cv_pileup_adopt_union(cv_pileup *p, int has_range, int64_t lo1, int64_t hi1, const int64_t *truth, int64_t ntruth,
                          void *stream, int64_t *n_out);
int cv_bamtrain_columns(const cv_pileup *p, const int32_t *depth_dev, const uint8_t *touched_dev, int64_t min_coverage,
                        int64_t *pos_dev, uint8_t *digits_dev, uint8_t *centre_dev, uint8_t *acgt_dev, uint8_t *flags_dev,
                        uint8_t *row_dev, void *stream);
int cv_bamtrain_pair(int64_t nrows, const int32_t *ctg_dev, const int64_t *pos_dev, const uint8_t *flags_dev,
                     const uint8_t *acgt_dev, const uint32_t *ctg_hash_dev, int32_t nctg, uint64_t seed, double amp,
                     uint8_t *keep_dev, int64_t *counts_dev, double *r_dev, void *stream);

/* One text row of CreateTensor.py (:52): "<ctg> <center> <seq33> " + 528 x "%0.1f" (no newline).
 * counts: [33,4,4] fp32 raw counts (host).  Returns the length written, or -1 if cap is small.  */
int64_t cv_format_tensor_row(const char *ctg, int64_t center, const char *seq, int64_t seqlen,
                             const float *counts, char *dst, int64_t cap);
/* The same rows written in HBM (csrc/cv_rowtext_dev.hip, cv_rowtext_core.hpp): row r is cv_format_tensor_row + "\n" of
 * centres_dev[r], counts_dev[r] ([rows,33,4,4] fp32) and the reference bytes [new_pos - 17, new_pos + 16) of the window
 * ref_dev[0, ref_len) whose first byte is 0-based position ref_first0 (new_pos = centre - ref_first0; the bytes as they
 * are, fewer than 33 where the window ends on either side), at text_dev + off_dev[r]; off_dev[rows + 1] int64, off_dev[rows] = bytes in all.
 * The device vouches only for what the host prints through its integer branch: a row with a value that is negative,
 * fractional, 2^24 or more, NaN or infinite, or with a centre < 1 gets
 * status_dev[r] = CV_ROWTEXT_HOST and length 0 (the caller formats it with cv_format_tensor_row); a contig name of more
 * than 255 bytes makes every row CV_ROWTEXT_HOST.  text_dev = NULL: lengths and status only, so that the caller can size
 * the text exactly and call again.  A row that would end behind text_cap is not written; nothing behind off_dev[rows]
 * is.  ctg is host memory; centres / off 8-byte, counts 16-byte, the workspace 256-byte aligned.  Asynchronous on
 * `stream`.                                                                                                          */
#define CV_ROWTEXT_DEVICE 0
#define CV_ROWTEXT_HOST 1
int cv_tensor_rows_text_workspace(int64_t rows, int64_t *bytes);
int cv_tensor_rows_text_dev(const char *ctg, int64_t ctg_len, const int64_t *centres_dev, int64_t rows,
                            const uint8_t *ref_dev, int64_t ref_first0, int64_t ref_len, const float *counts_dev,
                            int64_t *off_dev, uint8_t *status_dev, char *text_dev, int64_t text_cap,
                            void *workspace, int64_t workspace_bytes, void *stream);

/* The rows of ExtractVariantCandidates.py written in HBM (csrc/cv_candrows_dev.hip, cv_candrows_core.hpp); the host loop
 * candidate_rows of clairvoyante_amd/ExtractVariantCandidates.py stays the definition.
 *
 * cv_pileup_select_candidates: cv_pileup_extract_candidates' predicate and arguments, but the entries stay in HBM (as
 *   cv_pileup_sample_candidates leaves them) and only *n_out comes back; cv_pileup_get_extracted fetches them when asked.
 * cv_pileup_selected_dev: the n_out resident entries of the last cv_pileup_select_candidates / _sample_candidates gathered
 *   into the caller's device arrays (any may be NULL): pos0_dev[n] int64 0-based position, late_dev[n] int32, counts7_dev
 *   [n,7] int32 in A,C,G,T,I,D,N order; info (host) as cv_pileup_get_extracted fills it.  Nothing is copied to the host.
 * cv_candidate_order_dev: order_dev[n] int64 = the reference's output order of n ascending entries (candidate_order): the
 *   indices of the entries with late == 0 and pos0 < last_pos, ascending, then those of all others, ascending.
 * cv_candidate_rows_dev: output row r < rows is entry e = order_dev[r] (order_dev NULL: e = r) of the n entries:
 *     "<ctg> <pos0[e] + 1> <ref byte> <total> <S1> <c1> ... <S7> <c7>\n"
 *   total = the seven counts summed in 64 bits, the pairs by descending count, ties in the order A,C,G,T,I,D,N; the byte
 *   is ref_dev[pos0[e] - ref_first0] as it is.  The rows stand end to end at text_dev + off_dev[r]; off_dev[rows + 1]
 *   int64, off_dev[rows] = bytes in all.  text_dev = NULL: lengths and status only.  A row that would end behind text_cap
 *   is not written; nothing behind off_dev[rows] is.  The device vouches for a row only if e lies in [0, n), the position
 *   in [0, 2^63 - 2] and inside the window [ref_first0, ref_first0 + ref_len), the byte is below 0x80 and no count is
 *   negative: any other row gets status_dev[r] = CV_CANDROWS_HOST and length 0; a contig name of more than 255 bytes makes
 *   every row CV_CANDROWS_HOST.  late_dev is not read (a late entry differs in its counts alone) and may be NULL.  ctg is
 *   host memory; order / pos0 / off 8-byte, counts7 4-byte, the workspace 256-byte aligned; at most 2^30 rows and entries.
 * cv_candidate_rows_host_form: the same core on the CPU over HOST pointers.
 * The _dev calls are asynchronous on `stream`: no allocation, no synchronisation.                                      */
#define CV_CANDROWS_DEVICE 0
#define CV_CANDROWS_HOST 1
int cv_pileup_select_candidates(cv_pileup *p, double threshold, double min_coverage, int has_region, int64_t ctg_start,
                                int64_t ctg_end, const int64_t *bed_begin, const int64_t *bed_end, int64_t nbed,
                                void *stream, int64_t *n_out);
int cv_pileup_selected_dev(cv_pileup *p, int64_t *pos0_dev, int32_t *late_dev, int32_t *counts7_dev, int64_t info[2],
                           void *stream);
int cv_candidate_order_workspace(int64_t n, int64_t *bytes);
int cv_candidate_order_dev(const int64_t *pos0_dev, const int32_t *late_dev, int64_t n, int64_t last_pos, int64_t *order_dev,
                           void *workspace, int64_t workspace_bytes, void *stream);
int cv_candidate_rows_workspace(int64_t rows, int64_t *bytes);
int cv_candidate_rows_dev(const char *ctg, int64_t ctg_len, const int64_t *order_dev, int64_t rows, int64_t n,
                          const int64_t *pos0_dev, const int32_t *late_dev, const int32_t *counts7_dev,
                          const uint8_t *ref_dev, int64_t ref_first0, int64_t ref_len, int64_t *off_dev, uint8_t *status_dev,
                          char *text_dev, int64_t text_cap, void *workspace, int64_t workspace_bytes, void *stream);
int cv_candidate_rows_host_form(const char *ctg, int64_t ctg_len, const int64_t *order, int64_t rows, int64_t n,
                                const int64_t *pos0, const int32_t *late, const int32_t *counts7, const uint8_t *ref,
                                int64_t ref_first0, int64_t ref_len, int64_t *off, uint8_t *status, char *text,
                                int64_t text_cap);

/* callVarBam's columns written in HBM (csrc/cv_callcols_dev.hip, cv_callcols_core.hpp): which of the n candidate centres
 * give a row for the call loop, and the tokens of those rows.  Centre i (1-based, ri = centre - 1 - ref_first inside
 * the reference bytes ref[0, ref_len) whose first byte is 0-based position ref_first >= 0) is kept iff touched[i], ri - 16
 * >= 0, ri < ref_len and ref[ri], with a..z mapped to A..Z, is one of A, C, G, T.  For the k kept centres, in ascending
 * order of i (the compaction is stable):
 *   index [k] int64   i of the row
 *   text              the contig name, then the k coordinates ("%d", no separator), then the k windows
 *                     ref[ri - 16, min(ri + 17, ref_len)) with a..z mapped to A..Z and every other byte as it is -- 17 to 33
 *                     bytes each -- end to end: the bytes of utils_v2.PosBatch.from_columns
 *   meta [k,6] int64  offset and length of the contig name, the coordinate and the window of the row inside text
 *   info [4] int64    {k, bytes of text, n, 0}: k and the bytes are all a caller has to fetch
 * text_cap must be at least ctg_len + CV_CALL_COLUMNS_ROW_TEXT n (there is no sizing pass); nothing behind info[1] bytes
 * of text or behind row k of index / meta is written.  ctg is host memory, at most CV_CALL_COLUMNS_MAX_CTG bytes; the
 * centres 4-byte, index / meta / info 8-byte, the workspace 256-byte aligned; at most 2^27 centres.  A null or misaligned
 * pointer, a capacity below the bound or a negative ref_first returns 1.  Asynchronous on `stream`: no allocation, no
 * synchronisation, no host round trip.
 * cv_pileup_call_columns: the same behind cv_pileup_finish(touched_dev) for the handle's own centres and reference.
 * cv_call_columns_host_form: the same core on the CPU over HOST pointers (tests hold the kernels to it).            */
#define CV_CALL_COLUMNS_MAX_CTG 1024
#define CV_CALL_COLUMNS_ROW_TEXT 43
int cv_call_columns_workspace(int64_t n, int64_t *bytes);
int cv_call_columns_dev(const char *ctg, int64_t ctg_len, const int32_t *centres_dev, const uint8_t *touched_dev, int64_t n,
                        const uint8_t *ref_dev, int64_t ref_first, int64_t ref_len, int64_t *index_dev, int64_t *meta_dev,
                        char *text_dev, int64_t text_cap, int64_t *info_dev, void *workspace, int64_t workspace_bytes,
                        void *stream);
int cv_pileup_call_columns(const cv_pileup *p, const char *ctg, int64_t ctg_len, const uint8_t *touched_dev, int64_t *index_dev,
                           int64_t *meta_dev, char *text_dev, int64_t text_cap, int64_t *info_dev, void *workspace,
                           int64_t workspace_bytes, void *stream);
int cv_call_columns_host_form(const char *ctg, int64_t ctg_len, const int32_t *centres, const uint8_t *touched, int64_t n,
                              const uint8_t *ref, int64_t ref_first, int64_t ref_len, int64_t *index, int64_t *meta, char *text,
                              int64_t text_cap, int64_t *info);

/* ---- native `samtools view` (optional producer, host only) ------------------------------------
 * The text of `samtools view -F <exclude_flags> BAM CTG[:S-E]` (CreateTensor.py:128-130,
 * ExtractVariantCandidates.py:112-114) without the external process: BGZF blocks inflated by `threads`
 * host threads, records of the region printed as SAM lines (11 columns, QUAL '*' unless with_qual;
 * no auxiliary tags).  Uses BAM.bai / .bai (linear index) when present, otherwise scans from the start.
 * Formats per the SAM/BAM specification; validated against files written by tests/bam_writer.py.      */
typedef struct cv_bam cv_bam;
int cv_bam_open(const char *path, int threads, cv_bam **out);
void cv_bam_close(cv_bam *b);
int cv_bam_nref(const cv_bam *b);
int cv_bam_ref(const cv_bam *b, int i, const char **name, int64_t *len);
int cv_bam_has_index(const cv_bam *b);
/* beg1 / end1: 1-based inclusive region, both <= 0 for the whole contig.                              */
int cv_bam_view_begin(cv_bam *b, const char *ref, int64_t beg1, int64_t end1, int exclude_flags, int with_qual);
/* Whole SAM lines into buf[0, cap); returns bytes written (0 and *done = 1 at the end), -1 on error.   */
int64_t cv_bam_view_read(cv_bam *b, char *buf, int64_t cap, int *done);
/* The same selection without the text: the next run of selected records (about max_bytes of inflated BAM);
 * returns their count, record i starts at *base + (*offs)[i] with its refID field (SAM/BAM specification 4.2).
 * The pointers stay valid until the next call on the handle; 0 and *done = 1 at the end, -1 on error.
 * Feeds cv_pileup_add_bam.                                                                             */
int64_t cv_bam_view_records(cv_bam *b, int64_t max_bytes, const uint8_t **base, const uint32_t **offs, int *done);
/* CIGAR words of a record handed out by cv_bam_view_records (rec at refID): the inline ones, or the CG:B,I array
 * behind the long-read placeholder <l_seq>S<span>N (more than 65535 operations, SAMv1 4.2.2).  0 ok.      */
int cv_bam_record_cigar(const uint8_t *rec, const uint8_t **ops, int64_t *n);
/* ---- the BAM front end on the device (csrc/cv_bam_dev.hip, cv_bam_core.hpp; optional route of `--samtools native`) ----
 * The compressed BGZF members of a view go to the GPU; segments, SEQ bytes and flags are made in HBM and handed to the
 * pileup handle where cv_pileup_flush puts its uploads.  The host route (cv_bam_view_records + cv_pileup_add_bam) stays
 * the definition: same counters, same running state, same exception texts.  Needs the .bai.
 * cv_bam_view_plan_begin: cv_bam_view_begin without inflating anything; *usable = 0 when the file has no (intact)
 *   index or the index gives no start for the contig: the caller takes the host route.
 * cv_bam_view_plan: the next slab of the view -- a run of WHOLE members of about slab_bytes compressed bytes.
 *   info[0] members, [1] compressed bytes from *comp on (the first member's DEFLATE data to the last member's end),
 *   [2] inflated bytes, [3] offset in them of the first record to look at (first slab: voff & 0xffff of the start; 0
 *   afterwards, where the caller's carried tail goes in front), [4] anchors, [5] 1 = the file ends behind this slab,
 *   [6] file offset of the first member, [7] 1 = first slab of the view.  *table: rows as cv_bgzf_scan writes them
 *   (file offsets; cv_inflate_bgzf_dev takes them relative to the first row).  *anchors: the linear-index entries of the
 *   contig inside the slab and behind the start, distinct, ascending, as offsets in the slab's inflated bytes;
 *   duplicates, zeros, entries out of order or not at a member start of the slab are dropped (fewer walkers, never
 *   another result).  The pointers hold until the next call.  info[0] = 0: nothing left.
 * cv_bam_plan_inflate_host: member m of that slab inflated and CRC-checked on the host into dst (ISIZE bytes, <= 64 KiB);
 *   failure is the host route's "bam: corrupt BGZF block at offset N".
 * cv_bam_view_params: tid, exclude mask, beg0, end0 of the current view.
 * cv_bam_dev_view: the whole view through the device, slab by slab, into pileup handle p on `stream` (synchronises).
 *   A slab the device does not vouch for (a walker that misses its anchor, a placeholder CIGAR, a record that fails
 *   the layout checks, POS / CIGAR demands out of range) is refused before anything of p changes and goes to
 *   cv_pileup_add_bam from the same inflated bytes.  *kept = reads kept; counts[0] slabs, [1] records taken on the
 *   device, [2] members inflated on the device, [3] members inflated on the host, [4] slabs handed over to the host,
 *   [5] walkers that ran, [6] records of the slabs handed over, [7] members read.
 * cv_bam_dev_times: host wall time (ms, since creation) between the synchronisations of cv_bam_dev_view: [0] copy +
 *   inflate, [1] walk, [2] count + scans + running state, [3] emit + hand-over (with the pileup's own kernels), [4] slabs
 *   taken by the host; HIP-event time of [5] the inflate kernel and [6] the walk kernel alone.
 * cv_pileup_bam_params: out[0..4] = min_mq, dcov, evc, evc_min_mq, 1 if a contig is set; out[5..8] = prev_pos, depth_cap,
 *   evc_prev_pos, evc_reads (the running state of the depth cap and the late mark).
 * cv_pileup_add_bam_dev: a batch made on the device -- segs_dev[0, nseg) (20-byte segments in READ order, flags final,
 *   q0 absolute in seq_dev[0, nq)), `cols` alignment columns, state[4] the running state behind its last read.  Parts
 *   queued on the host are flushed first; then evc_count / pileup_scatter / retention exactly as cv_pileup_flush.
 * cv_pileup_reserve_bam_dev: the place of that batch in the handle (room for nseg >= 1 segments, nq + 64 SEQ bytes; the
 *   host queue is flushed here), so that it is written where the kernels read it: cv_pileup_add_bam_dev with these
 *   pointers takes it without a copy, with other pointers it copies device to device.                               */
typedef struct cv_bam_dev cv_bam_dev;
int cv_bam_view_plan_begin(cv_bam *b, const char *ref, int64_t beg1, int64_t end1, int exclude_flags, int *usable);
int cv_bam_view_plan(cv_bam *b, int64_t slab_bytes, int64_t info[8], const uint8_t **comp, const int64_t **table,
                     const int64_t **anchors);
int cv_bam_plan_inflate_host(cv_bam *b, int64_t m, uint8_t *dst);
int cv_bam_view_params(const cv_bam *b, int64_t out[4]);
int cv_bam_dev_create(int device, cv_bam_dev **out);
void cv_bam_dev_destroy(cv_bam_dev *d);
int cv_bam_dev_view(cv_bam_dev *d, cv_bam *b, cv_pileup *p, int64_t slab_bytes, int contig_ok, void *stream, int64_t *kept,
                    int64_t counts[8]);
int cv_bam_dev_times(const cv_bam_dev *d, double ms[7]);
int cv_pileup_bam_params(const cv_pileup *p, int64_t out[9]);
int cv_pileup_reserve_bam_dev(cv_pileup *p, int64_t nseg, int64_t nq, void **segs_dev, uint8_t **seq_dev, void *stream);
int cv_pileup_add_bam_dev(cv_pileup *p, const void *segs_dev, int64_t nseg, const uint8_t *seq_dev, int64_t nq, int64_t cols,
                          const int64_t state[4], void *stream);
/* The block decoder behind the BGZF reader (raw DEFLATE, RFC 1951, whole block in memory): src[0, n) must be
 * followed by 8 readable bytes, the stream must produce exactly cap bytes; returns cap or -1.  And the CRC-32 of
 * the gzip trailer (start with crc = 0).                                                                 */
int64_t cv_inflate_raw(const uint8_t *src, int64_t n, uint8_t *dst, int64_t cap);
/* The same decoder over a gzip member too large to inflate at once (text-tensor files, utils_v2.GetTensor -- the
 * reference pipes them through `gzip -fdc`, utils_v2.py:25): src[0, n) = the raw-DEFLATE data behind the gzip header,
 * followed by >= 8 readable bytes; *bitpos = bit offset to go on from (0 first); dst[0, have) = the output produced
 * last (>= its last 32 768 bytes), new output is appended at dst + have up to dst + cap.  Returns at the first block
 * boundary with >= want new bytes or at the end of the stream (*final = 1; the CRC-32 / ISIZE trailer starts at the
 * byte boundary behind *bitpos): the number of new bytes, or -1 (malformed / a block that does not fit).          */
int64_t cv_inflate_stream(const uint8_t *src, int64_t n, int64_t *bitpos, uint8_t *dst, int64_t have, int64_t cap,
                          int64_t want, int32_t *final);
uint32_t cv_crc32_ieee(uint32_t crc, const uint8_t *p, int64_t n);

/* ---- chunk VCFs merged on the device (csrc/cv_vcfmerge_dev.hip, csrc/cv_vcfmerge_core.hpp) ----------------------------
 * The last line of the whole-genome recipe (vcfcat | vcfstreamsort | bgziptabix): clairvoyante_amd/vcf_merge.py holds the
 * definition.  text_dev[0, text_len) = the record bytes of all inputs end to end, 16-byte aligned and readable up to the
 * next multiple of 16 behind text_len; pos / run / off / len = the n rows of cv_item_lines_dev over it (every line a ROW);
 * run_rank_dev[nruns] = the contig rank (0 .. nrank - 1) of each run.
 *
 * cv_vcf_merge_dev: a line is vouched for unless it has fewer than 8 tab-separated columns, its first two columns are not
 * "token TAB digits TAB", INFO holds an END= key (at its start or behind a ';'), REF is empty, POS < 1 or POS - 1 +
 * len(REF) > 2^29, or its row lies outside the text / its run outside the ranks.  The records are ordered by (rank, POS,
 * line number) -- one stable radix sort over the key bits the data needs --, and in that order:
 *   srank_dev[i] int32, sbeg_dev[i] = POS - 1, send_dev[i] = sbeg + len(REF), ooff_dev[n + 1] = the offset of record i in
 *   the output (an exclusive sum of the lengths; ooff[n] = the bytes in all);
 *   out_text_dev[0, ooff[n]) the sorted text (may be NULL: no text; a range that does not fit below out_cap is not written);
 *   chunks_dev[4][n] = rank, bin, ubeg, uend of the info[1] chunks -- the maximal runs of equal (rank, reg2bin) --
 *   sorted by (rank, bin), in file order within a bin;
 *   stats_dev[4][nrank] = per rank the offset of its first record, the offset behind its last, its records, its largest end;
 *   info_dev[8] = {lines not vouched for, chunks, bytes, 0 ...}.  With info[0] != 0 nothing else is to be used: the
 *   call is the host loop's.  At most 2^30 records and 2^20 ranks.
 * cv_vcf_windows_dev: win_dev[win_off[r] + w] = the smallest ooff of a record of rank r that overlaps window w of 16 384
 * bp, a window no record touches taking the next one's value (the linear index, back-filled); win_off_dev[nrank + 1] is
 * the caller's (n_intv per rank from stats), windows outside it are not written.  Needs no workspace.
 * The _host_form twins: the same core on the CPU over HOST pointers.  The _dev calls are asynchronous on `stream`: no
 * allocation, no synchronisation; the workspace is 256-byte aligned.                                                     */
int cv_vcf_merge_workspace(int64_t n, int64_t *bytes);
int cv_vcf_merge_dev(const char *text_dev, int64_t text_len, int64_t n, const int64_t *pos_dev, const int32_t *run_dev,
                     const int64_t *off_dev, const int64_t *len_dev, const int32_t *run_rank_dev, int64_t nruns, int32_t nrank,
                     int32_t *srank_dev, int64_t *sbeg_dev, int64_t *send_dev, int64_t *ooff_dev, char *out_text_dev,
                     int64_t out_cap, int64_t *chunks_dev, int64_t *stats_dev, int64_t *info_dev, void *workspace_dev,
                     int64_t workspace_bytes, void *stream);
int cv_vcf_merge_host_form(const char *text, int64_t text_len, int64_t n, const int64_t *pos, const int32_t *run,
                           const int64_t *off, const int64_t *len, const int32_t *run_rank, int64_t nruns, int32_t nrank,
                           int32_t *srank, int64_t *sbeg, int64_t *send, int64_t *ooff, char *out_text, int64_t out_cap,
                           int64_t *chunks, int64_t *stats, int64_t *info);
int cv_vcf_windows_dev(int64_t n, const int32_t *srank_dev, const int64_t *sbeg_dev, const int64_t *send_dev,
                       const int64_t *ooff_dev, int32_t nrank, const int64_t *win_off_dev, int64_t *win_dev, int64_t nwin,
                       void *stream);
int cv_vcf_windows_host_form(int64_t n, const int32_t *srank, const int64_t *sbeg, const int64_t *send, const int64_t *ooff,
                             int32_t nrank, const int64_t *win_off, int64_t *win, int64_t nwin);

/* ---- BGZF members compressed on the device (csrc/cv_bgzf_deflate_dev.hip, csrc/cv_bgzf_deflate_core.hpp) ---------------
 * The writer's side of utils_v2.BgzfWriter (deflate="device"): text_dev[0, len) -- any alignment -- is cut every `block`
 * bytes (1 .. 65 280); member k holds the bytes [k * block, min(len, (k + 1) * block)) as the 18-byte BGZF header with
 * BSIZE, ONE final DEFLATE block -- the smallest of stored, fixed and dynamic Huffman, from a position-parallel match
 * search and a greedy parse -- and the CRC-32 / ISIZE trailer.  An empty text is one empty member.  The members lie back to
 * back in out_dev[0, info[0]); a member that does not fit below out_cap is not written.  No member is larger than its
 * stored form, len_k + 31 bytes, so members * (block + 31) always suffices.
 *   sizes_dev[members] int32 = the bytes of each member, header and trailer included;
 *   info_dev[8] = {bytes of all members, members, stored, fixed, dynamic, 0 ...}.
 * The bytes are those of cv_bgzf_deflate_host_form, the same core on the CPU over HOST pointers, and depend on nothing but
 * the text and the block.  They are NOT zlib's: any inflater is the judge.  Asynchronous on `stream`: no allocation, no
 * synchronisation; the workspace is 256-byte aligned.                                                                    */
int cv_bgzf_deflate_workspace(int64_t members, int64_t block, int64_t *bytes);
int cv_bgzf_deflate_dev(const uint8_t *text_dev, int64_t len, int64_t block, uint8_t *out_dev, int64_t out_cap, int32_t *sizes_dev,
                        int64_t *info_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
/* one of the three launches alone (0 compress, 1 offsets, 2 assemble), for the probe's HIP events; after one whole call */
int cv_bgzf_deflate_phase_dev(int phase, const uint8_t *text_dev, int64_t len, int64_t block, uint8_t *out_dev, int64_t out_cap,
                              int32_t *sizes_dev, int64_t *info_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int cv_bgzf_deflate_host_form(const uint8_t *text, int64_t len, int64_t block, uint8_t *out, int64_t out_cap, int32_t *sizes,
                              int64_t *info);

#ifdef __cplusplus
}
#endif
#endif /* CLAIRVOYANTE_AMD_H */
