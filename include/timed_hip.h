/*
 * timed_hip.h — C ABI of libtimedhip.so, the MI355X (gfx950) engine behind the reference's two
 * numeric seams.  Plain pointers and sizes only; no C++/torch types; never throws across the ABI.
 *
 * The reference (wells-wood-research/timed-design) has no FFI/plugin layer: the seams are Python
 * call sites.  Each entry point below names the reference interface it replaces (file:line are
 * relative to the reference repo).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every function returns 0 (TH_OK) or a negative TH_E* code; th_last_error() returns a
 *     thread-local human-readable message for the last failure on the calling thread.
 *   - the caller owns every host buffer; the library owns device buffers it allocates.
 *   - threading: a th_model handle is bound to one device.  Submissions on one handle (th_predict,
 *     th_predict_async, th_predict_device) are serialised by a lock inside the handle, and
 *     th_predict_wait may be called from a DIFFERENT thread than the one that submitted the ticket
 *     (predict.py waits on its writer thread while the main thread keeps submitting): a ticket slot
 *     is only handed out again after its waiter has returned, whether it succeeded or failed.  One
 *     waiter per ticket (a second concurrent wait on the same ticket gets TH_EBUSY).  th_model_free,
 *     th_model_set_chunk and th_model_profile must not run concurrently with anything else on the
 *     handle.  Distinct handles may be driven from distinct threads (ctypes releases the GIL).
 *   - frames are channels-last [n, D, H, W, C], C fastest — the layout
 *     design_utils/utils.py:519-527 (load_batch) builds and Keras consumes.
 */
#ifndef TIMED_HIP_H
#define TIMED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TH_OK 0
#define TH_EINVAL (-1)   /* bad argument / shape / dtype                     */
#define TH_EIO (-2)      /* pack file unreadable or malformed                */
#define TH_EHIP (-3)     /* a HIP runtime call failed (message has details)  */
#define TH_EUNSUP (-4)   /* layer/option outside the supported op set        */
#define TH_ENOMEM (-5)
#define TH_ECOMM (-6)    /* RCCL failure / librccl.so not loadable           */
#define TH_EBUSY (-7)    /* every async ticket of the model is in flight     */

/* element types accepted for frames (what load_batch can hand to Model.predict,
 * design_utils/utils.py:518-521: float64 when voxels_as_gaussian else bool) */
#define TH_F32 0
#define TH_F64 1
#define TH_U8 2
#define TH_BOOL 3
#define TH_F16 4

/* th_model_load flags */
#define TH_LOAD_DEFAULT 0u
#define TH_LOAD_NO_FUSE 1u      /* one kernel per Keras layer (debug / parity bisecting)          */
#define TH_LOAD_NO_MFMA 2u      /* direct (VALU) convolution kernels only                         */
#define TH_LOAD_KEEP_ALL 4u     /* keep every layer output materialised (th_model_fetch)          */

/* th_predict* flags */
#define TH_PREDICT_DEFAULT 0u
#define TH_PREDICT_LOGITS 1u    /* skip the final Softmax: return its input (parity on the logits) */
#define TH_PREDICT_OUT_DEVICE 2u /* th_predict/_async: probs_out is memory of the model's DEVICE (frames still come from the
                                  * host); the rows stay in HBM, e.g. for th_comm_gather_rows */
#define TH_PREDICT_IN_DEVICE 4u  /* th_predict/_async: `frames` is memory of the model's DEVICE already (e.g. frames that
                                  * th_h5_decode_device inflated there): no host->device copy; it must stay valid until the wait */

typedef struct th_model th_model;
typedef struct th_comm th_comm;

/* ---- library ---------------------------------------------------------------------------- */
int th_version(void);                 /* ABI version, currently 1 */
const char* th_last_error(void);
int th_device_count(int* n_out);
/* CPUs the host-side thread pools of this library will use: min(hardware threads, affinity, cgroup CPU quota) */
int th_host_cpus(void);
/* name/arch of a device, e.g. "AMD Instinct MI355X" / "gfx950" */
int th_device_info(int device, char* name, size_t name_len, char* arch, size_t arch_len, int* cus);

/* ---- model: replaces tf.keras.models.load_model(path) — predict.py:121 ------------------- */
/* `pack_path` is a THPK0001 pack written by timed_hip/pack.py from the .h5's model_config+weights */
int th_model_load(const char* pack_path, int device, unsigned flags, th_model** out);
int th_model_load_mem(const void* pack, size_t nbytes, int device, unsigned flags, th_model** out);
void th_model_free(th_model* m);
/* input dims {D,H,W,C} (= dataset attr frame_dims, utils.py:515) and width of the output row */
int th_model_info(const th_model* m, int dims[4], int* n_classes);
/* algorithmic work per frame: FLOPs (2*V*k^3*Cin*Cout per conv + 2*F*out per Dense) and the
 * executed FLOPs including tile padding; number of device launches per chunk */
int th_model_cost(const th_model* m, double* algo_flops, double* exec_flops, int* n_steps);
/* frames processed per internal pass (Keras' own predict() minibatch is 32 — no numeric effect) */
int th_model_set_chunk(th_model* m, int frames_per_chunk);
/* 16-row tiles per wave, 1 or 2, that the batch-row convolution kernel (k_conv_gl) runs with when one launch covers `rows` GEMM rows
 * (rows = frames in the chunk x output voxels per frame).  The results do not depend on it; tests call the rule so that they do not
 * copy it.  Host code. */
int th_conv_gl_row_tiles(int64_t rows);
/* The dispatch rule of the pointwise (1x1x1) kernels, for tests.  th_conv_pw_pick writes the name of the instantiation that runs a
 * Cin -> Cout layer (pool: 0 none, 1 max, 2 avg) on an input view of voxel stride in_cs floats (<= 0: Cin) at channel offset
 * in_coff, with chunk-blocked output or not, behind a "BN-affine -> ReLU" epilogue or not: "k_conv_pw2<12,2,0,1,2>",
 * "k_conv_pw<16,4,0>"; the empty string when the pointwise family refuses the layer.  th_conv_pw_kernels lists every compiled
 * instantiation, one name per line. */
int th_conv_pw_pick(int Cin, int Cout, int pool, int in_cs, int in_coff, int out_blk, int relu_chain, char* buf, size_t len);
int th_conv_pw_kernels(char* buf, size_t len);
/* The planner's rule for the two brick kernels (k_conv_n16, k_conv_mfma), for tests.  th_conv_brick_pick writes the plan label of a
 * kd x kh x kw convolution Cin -> Cout with this stride and dilation, Keras 'same' (same != 0) or 'valid' padding, on a D x H x W volume
 * with a fused 2x2x2 pool (0 none, 1 max, 2 avg; one pool value, as the planner tries it), read from an input view of voxel stride
 * in_cs floats (<= 0: a dense tensor) at channel offset in_coff:
 * "conv_mfma<w8,4x2,nt2,ci16,stream,pool1> FB1 ZB6/12 rows96 lds150K [k_conv_mfma<8,4,2,2,16,2,1,0>]", two such labels joined by
 * " x2 + " when the last block of output channels runs on a narrower instantiation, the empty string when neither kernel plans the
 * layer.  Default knobs.  th_conv_brick_kernels lists every compiled instantiation of both kernels, one name per line.  Host code. */
int th_conv_brick_pick(int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, const int stride[3], const int dilation[3],
                       int same, int pool, int in_cs, int in_coff, char* buf, size_t len);
int th_conv_brick_kernels(char* buf, size_t len);

/* ---- forward: replaces frame_model.predict(X_batch) — predict.py:142 --------------------- */
/* host frames [n,D,H,W,C] of `dtype` -> host probs_out [n,n_classes] fp32 (rows sum to 1) */
int th_predict(th_model* m, const void* frames, int dtype, int64_t n, float* probs_out, unsigned flags);
/* The same call split in two so that the caller's loop (the per-batch loop of predict.py:125-155, whose load_batch
 * — design_utils/utils.py:487-530 — re-opens the dataset and gathers the next batch on the host) overlaps with the GPU:
 * th_predict_async queues host->device copy, kernels and the device->host copy of the probabilities and returns a
 * ticket; th_predict_wait blocks until that batch is complete and only then writes probs_out.  Up to 4 tickets per
 * model may be in flight (TH_EBUSY beyond that); they complete in submission order.  `frames` must stay valid and
 * unmodified until the matching th_predict_wait returns.  Frames in page-locked memory (th_host_alloc /
 * th_host_register) are copied by the DMA engine without blocking the caller; with pageable memory the copy of a piece
 * blocks the caller (the kernels of earlier pieces and tickets still run underneath it).  th_predict ==
 * th_predict_async + th_predict_wait. */
int th_predict_async(th_model* m, const void* frames, int dtype, int64_t n, float* probs_out, unsigned flags, int* ticket);
int th_predict_wait(th_model* m, int ticket);
/* Lossless sparse transport of float32 frames (row f-1: what design_utils/utils.py:487-530 hands to Model.predict, predict.py:142).
 * Gaussian aposteriori frames are ~8 % non-zero; over PCIe a frame then costs ~25 KB instead of 222 KB, and is rebuilt bit for bit
 * on the device in front of the first layer.  `blob` (host memory, little-endian, 16-byte aligned) is
 *     0   char     magic[8] = "THSPF001"
 *     8   uint32   n_frames, elems_per_frame E, bitmap words per frame W (>= ceil(E / 32), a multiple of 4), element bytes (4)
 *     24  uint64   n_values
 *     32  uint64   rank[n_frames + 1]      stored elements in front of frame i (rank[n] - rank[0] = n_values)
 *     ..  (to the next multiple of 16)
 *         uint32   bitmap[n_frames][W]     bit k of word w set <=> element 32 w + k is stored (every element whose bit pattern is
 *                                          not +0.0: -0.0, NaN payloads and denormals are stored)
 *         float    values[n_values]        the stored elements, frame by frame, in element order
 * The whole blob is checked on the host before anything is queued: W <= 4096 (131 072 elements per frame), n_values within
 * blob_bytes, and for every frame popcount(bitmap[i]) == rank[i + 1] - rank[i] with no bit set at or beyond element E (the tail
 * of the last real word, the padding words).  A blob that fails returns TH_EINVAL (the message names the frame), takes no
 * ticket and writes nothing to probs_out.
 * Same ticket / wait / ownership rules as th_predict_async (TH_PREDICT_LOGITS and TH_PREDICT_OUT_DEVICE apply). */
#define TH_SPARSE_MAGIC "THSPF001"
int th_predict_sparse_async(th_model* m, const void* blob, size_t blob_bytes, float* probs_out, unsigned flags, int* ticket);
/* page-locked host memory for frame batches (what load_batch fills): allocate, or pin an existing range in place */
int th_host_alloc(size_t bytes, void** out);
int th_host_free(void* p);
int th_host_register(void* p, size_t bytes);
int th_host_unregister(void* p);
/* same with frames and probabilities already resident in this model's device memory */
int th_predict_device(th_model* m, const void* d_frames, int dtype, int64_t n, float* d_probs, unsigned flags);
/* copy a layer's output for the first n frames of the LAST chunk run (TH_LOAD_KEEP_ALL / unfused
 * layers only): out is [n, D,H,W,C] or [n,F] fp32.  Debug/parity aid. */
int th_model_fetch(th_model* m, const char* layer_name, int64_t n, float* out, int64_t out_floats);

/* per-launch timing with HIP events on the model's stream, accumulated over th_predict* calls until the
 * next th_model_profile call: enable = 0 off, 1 every step of the plan, 2 only the step with the most
 * algorithmic FLOPs (2 events per chunk: negligible cost inside a timed region) */
int th_model_profile(th_model* m, int enable);
/* step i of the plan: kernel label, accumulated ms and launch count since profiling was enabled,
 * algorithmic FLOPs and bytes per frame attributed to the step */
int th_model_step_info(const th_model* m, int i, char* label, size_t label_len, double* ms, int64_t* launches,
                       double* flops_per_frame, double* exec_flops_per_frame, double* bytes_per_frame);
/* the SURVEY §8(d) direct-form FLOPs per frame of step i when they differ from what the step's kernel computes (Cook-Toom /
 * Winograd steps: flops_per_frame of th_model_step_info is their own, smaller count); -1 for every other step */
int th_model_step_direct_flops(const th_model* m, int i, double* direct_flops_per_frame);

/* Load-time guard.  th_model_load checks the plan it built — Winograd layers, the bf16x3-split GEMMs — against a direct fp32-MFMA
 * plan of the same pack on four internally generated frames: the logits must agree to 1e-5 x max(1, max |logit|).  If they do
 * not, fast features are dropped (split GEMM, 5^3 Winograd, fused 10^3 Winograd, first-layer F(2,3), in that order) until they
 * do.  state: 0 not run (TH_GUARD=0 or nothing to check), 1 passed, 2 tripped — `note` then says what was measured and dropped.
 * max_dlogit: the kept plan's distance from the direct plan; logit_scale: max |logit| of the direct plan on the guard frames. */
int th_model_guard_info(const th_model* m, int* state, double* max_dlogit, double* logit_scale, char* note, size_t note_len);

/* the A/B and test knobs (TH_* environment variables) this handle was loaded under, as "NAME=value ..." — empty when every
 * knob had its default.  They are read once, by th_model_load, and never again (a later setenv does not reach a loaded handle). */
int th_model_knobs(const th_model* m, char* buf, size_t buf_len);

/* ---- device memory helpers (so host code needs no torch/hip-python for resident buffers) -- */
int th_dev_alloc(int device, size_t bytes, void** d_out);
int th_dev_free(int device, void* d);
int th_dev_upload(int device, void* d_dst, const void* h_src, size_t bytes);
int th_dev_download(int device, void* h_dst, const void* d_src, size_t bytes);
int th_dev_sync(int device);
/* fill d_frames [n,side,side,side,channels] fp32 with synthetic Gaussian-splat frames generated on
 * the device (Philox; statistically like timed_hip.synth.synthetic_frames, not bit-identical) */
int th_dev_synth_frames(int device, float* d_frames, int64_t n, int side, int channels, int atoms, uint64_t seed);

/* ---- sampler: replaces design_utils/sampling_utils.py ------------------------------------- */
/* apply_temp_to_probs (sampling_utils.py:139-161): q = p**(1/t), rows renormalised; fp64 */
int th_apply_temp(const double* probs, int64_t n_res, int n_cls, double t, double* out);           /* device 0 */
int th_apply_temp_on(int device, const double* probs, int64_t n_res, int n_cls, double t, double* out);
/* random_choice_prob_index (sampling_utils.py:53-90, kernel lines 81-82), n_samples draws fused:
 *   idx[s,i] = first j with cumsum_j(q[i,:]) > r[s,i], 0 if none   (q = tempered probs, t==1: q=p)
 * rng_mode 0: r = uniforms[s*n_res+i] supplied by the caller (e.g. np.random.rand — bit-exact
 *             replay of the reference's MT19937 stream);
 * rng_mode 1: r drawn on the device: rocRAND Philox4x32-10, seed, subsequence s*n_res+i;
 * rng_mode 2: r drawn on the device from MT19937 seeded like np.random.seed(seed), consumed in the
 *             reference's single-process order (for s: r = rand(n_res)). */
#define TH_RNG_HOST 0
#define TH_RNG_PHILOX 1
#define TH_RNG_MT19937 2
#define TH_RNG_MT_WORDS 3 /* th_sampler_run only: `uniforms` holds RAW MT19937 state words (uint32, two per draw, as th_mt19937_words
                           * returns them); the draw kernel tempers them and forms genrand_res53 itself — the doubles are the ones
                           * np.random.rand returns, the host only advances the recurrence */
int th_sample(const double* probs, int64_t n_res, int n_cls, int64_t n_samples, double temperature,
              int rng_mode, uint64_t seed, const double* uniforms, int32_t* idx_out);               /* device 0 */
/* optionally also return the uniforms the device drew (r_out [n_samples,n_res], may be NULL) and
 * residue letters (letters_out [n_samples, n_res] bytes, via cat_letters[n_cls], may be NULL) */
/* rng_offset = uniforms already consumed from the device stream (Philox: added to the subsequence
 * index; MT19937: doubles skipped) so successive calls continue one stream, as the reference's
 * per-PDB loop does.  q_out (may be NULL) receives the tempered probabilities [n_res,n_cls]. */
int th_sample_ex(const double* probs, int64_t n_res, int n_cls, int64_t n_samples, double temperature,
                 int rng_mode, uint64_t seed, uint64_t rng_offset, const double* uniforms, int32_t* idx_out,
                 double* r_out, const char* cat_letters, char* letters_out, double* q_out, int device);

/* A resident sampler: the probability rows of a whole run (every PDB key of sample.py's prediction matrix) stay on
 * one device, tempered and normalised, with their running sums; any number of sequences for any contiguous range of
 * keys is then drawn by ONE launch sequence — instead of one upload + launch + synchronise per key as the per-PDB
 * loop of sample_with_multiprocessing (sampling_utils.py:164-197) would do.  A handle serialises its own calls. */
typedef struct th_sampler th_sampler;
int th_sampler_create(int device, th_sampler** out);
void th_sampler_free(th_sampler* s);
#define TH_TEMPER_NONE 0        /* rows used as they are (sample.py:40 skips apply_temp_to_probs at T == 1)        */
#define TH_TEMPER_POW 1         /* q = p**(1/t), rows renormalised (sampling_utils.py:159-161)                      */
#define TH_TEMPER_PREPOWERED 2  /* rows already hold p**(1/t) (powered by the caller's NumPy); rows renormalised    */
/* probs [n_rows, n_cls] fp64 (host).  TH_TEMPER_POW: exponents 1, 2 and 0.5 are exact IEEE operations on the device
 * (NumPy takes the same fast paths); any other exponent is raised on the HOST with libm pow() before the upload —
 * device pow() is not correctly rounded and one ulp in q can move a residue index.  NumPy's own float64 `**` is libm
 * pow() in its scalar loop but an SVML routine under AVX-512, which differs in the last bit for ~5 % of inputs: a
 * caller that must reproduce one particular NumPy build bit for bit powers the rows itself and passes
 * TH_TEMPER_PREPOWERED (design_utils.sampling_utils does).  The normaliser follows NumPy's pairwise summation order
 * and the running sum is strictly sequential.  q_out (may be NULL) receives the tempered rows.
 * cum_dtype (TH_F64, TH_F32 or TH_F16) is the type the running sum is rounded to after every addition: np.cumsum
 * accumulates in the array's own dtype and the reference passes predict's float16 rows unconverted
 * (sampling_utils.py:82,125); sample.py's own path is float64. */
int th_sampler_load(th_sampler* s, const double* probs, int64_t n_rows, int n_cls, double temperature, int temper_mode,
                    int cum_dtype, double* q_out);
/* Key k owns rows [row_off[k], row_off[k+1]) of the loaded matrix (row_off has n_keys+1 ascending entries).  Draws are
 * numbered in the reference's consumption order — for key: for sample: rand(n_res_key) (sampling_utils.py:118-125):
 *   d(k, s, i) = n_samples*(row_off[k]-row_off[0]) + s*n_res_k + i
 * which is the position of the draw's uniform in `uniforms` (TH_RNG_HOST) or in the device stream (offset by
 * rng_offset), and of its result in idx_out / r_out / letters_out (each may be NULL).  cat_letters[n_cls] maps a
 * category to its one-letter code.  metrics_out (may be NULL) receives, per sampled sequence in the same key-major
 * order, [charge at pH 7.4, isoelectric point, molecular weight, molar extinction at 280 nm] — the tuple
 * calculate_seq_metrics (design_utils/analyse_utils.py:351-371) appends to every sequence at sampling_utils.py:132;
 * computed on the device from a 20-bin residue histogram per sequence (constants: ampal's published tables as
 * restated in design_utils/analyse_utils.py — parity unpinned, ampal is not in the reference tree). */
int th_sampler_draw(th_sampler* s, int64_t n_keys, const int64_t* row_off, int64_t n_samples, int rng_mode, uint64_t seed,
                    uint64_t rng_offset, const double* uniforms, const char* cat_letters, int32_t* idx_out, double* r_out,
                    char* letters_out, double* metrics_out);

/* A whole sample.py run in ONE submission (reference sampling_utils.py:118-133 for every key at once): the rows [n_rows, n_cls]
 * are used as they are (sample.py tempers the matrix first, sample.py:40-41), their running sums (in cum_dtype), every draw, the
 * one-letter codes and the per-sequence metrics are computed by two kernels between ONE host->device copy (rows, offsets and
 * letters travel together) and ONE device->host copy; caller-supplied uniforms (TH_RNG_HOST) add the copy of those.  Keys must
 * cover rows 0..n_rows.  want: bit 0 indices (int32 [total]), bit 1 letters (char [total]), bit 2 metrics (double [n_keys *
 * n_samples][4]) — in th_sampler_draw's draw order.  *block_out points at a page-locked block owned by the sampler (valid until
 * its next call); offsets_out[0..2] = byte offset of indices / letters / metrics in it, -1 when not requested.  Indices and
 * letters are bit-identical to th_sampler_load + th_sampler_draw on the same rows, uniforms / generator settings. */
/* a page-locked buffer of at least `bytes` owned by the sampler (grow-only, valid until the next call of this function on it or
 * th_sampler_free): uniforms or raw generator words written here reach the device by direct DMA instead of through HIP's
 * pageable staging copy */
int th_sampler_uniform_buffer(th_sampler* s, size_t bytes, void** out);
int th_sampler_run(th_sampler* s, const double* probs, int64_t n_rows, int n_cls, int cum_dtype, int64_t n_keys, const int64_t* row_off,
                   int64_t n_samples, int rng_mode, uint64_t seed, uint64_t rng_offset, const double* uniforms, const char* cat_letters,
                   unsigned want, const void** block_out, int64_t* offsets_out);

/* np.random.rand(n) of NumPy's GLOBAL legacy generator — the reference's source of uniforms, r = np.random.rand(n),
 * sampling_utils.py:81 — replayed natively (host code): key = the 624 MT19937 state words and *pos the position in them, as
 * np.random.get_state() returns them; out receives the same n doubles (genrand_res53) NumPy would produce and key / *pos are left
 * as NumPy would leave them, so np.random.set_state((name, key, pos, has_gauss, cached)) continues the stream seamlessly. */
int th_mt19937_rand(uint32_t* key, int* pos, int64_t n, double* out);
/* the same walk through the generator, but `out` receives the 2 n RAW state words the n doubles are made of (untempered, in
 * consumption order: double i = res53(temper(out[2 i]) >> 5, temper(out[2 i + 1]) >> 6)); key / *pos advance exactly as in
 * th_mt19937_rand.  For TH_RNG_MT_WORDS: the recurrence stays on the host (it is sequential), tempering and conversion — two
 * thirds of th_mt19937_rand's time — move into the draw kernel. */
int th_mt19937_words(uint32_t* key, int* pos, int64_t n, uint32_t* out);

/* ---- text output: replaces np.savetxt(f, matrix, delimiter=",") — design_utils/utils.py:768-771 (float16
 * probabilities) and predict.py:145-146 (full-precision rotamer matrix).  Host code only.  Formats the row-major
 * [n, k] matrix exactly as NumPy does (every value '%.18e', ',' between columns, '\n' after each row, NaN as
 * 'nan') into out; dtype is TH_F16 (preformatted table), TH_F32 or TH_F64.  Returns the number of bytes written,
 * or a negative TH_E* code (cap too small: 28 bytes per value always suffice). */
int64_t th_format_csv(const void* data, int dtype, int64_t n, int64_t k, char* out, int64_t cap);
/* The same text for a float32 matrix, formatted ON THE DEVICE (one lane per value): np.savetxt(f, y_pred_batch, delimiter=",") of
 * predict.py:145-146 — the full-precision rotamer matrix, 338 values per residue, ~1 GB of text per 125 000 residues.  rows: host
 * memory, [n, k] float32; out: host memory, cap >= 25 n k.  Every finite non-negative float32 below 2^24 (every probability) is
 * exactly 24 characters in '%.18e' form, so the text is 25 n k bytes (returned).  TH_EUNSUP when a value does not have that form
 * (negative, NaN, infinite, >= 2^24): the caller formats the block with th_format_csv instead — same bytes for every value both
 * accept (csrc/fmt_e18_f32.h is compiled for host and device).  Keeps a stream and two device buffers for `device` between calls;
 * th_format_csv_device_release gives them back.  Serialised internally (one formatter per process). */
int64_t th_format_csv_device(int device, const float* rows, int64_t n, int64_t k, char* out, int64_t cap);
int th_format_csv_device_release(void);
/* dataset-map text -> string table: replaces np.genfromtxt(dataset_map_path, delimiter=",", dtype="str") — predict.py:99.
 * th_csv_shape validates plain ASCII text with the same number of `delim`-separated, non-empty fields on every line and
 * reports (rows, cols, longest field); TH_EUNSUP for anything NumPy treats specially (comments, quotes, '\r', non-ASCII,
 * ragged or blank lines, blank-padded fields): the caller then falls back to NumPy.  th_csv_fill writes the fields as
 * UCS-4 code units into out[rows][cols][width], zero padded — the memory of a NumPy '<U{width}' array.  Host code. */
int th_csv_shape(const char* text, int64_t len, char delim, int64_t* rows_out, int* cols_out, int* width_out);
int th_csv_fill(const char* text, int64_t len, char delim, int64_t rows, int cols, int width, uint32_t* out);
/* argmax + residue letter per row: replaces max_idx = np.argmax(prediction_matrix, axis=1) and the per-residue string
 * appends of extract_sequence_from_pred_matrix — design_utils/utils.py:659, :689-692.  matrix [n, k] of dtype TH_F16 /
 * TH_F32 / TH_F64; np.argmax rules (first maximum; the first NaN of a row wins).  letters_out[i] = col_letters[argmax_i]
 * (col_letters: k bytes, the one-letter code of every probability column); idx_out (int32[n]) optional; either output
 * may be NULL.  Host code, rows split over host threads. */
int th_argmax_letters(const void* matrix, int dtype, int64_t n, int64_t k, const char* col_letters, char* letters_out,
                      int32_t* idx_out);

/* ---- evaluation: predict.py --output_analysis — what the reference computes with sklearn / scipy in
 * design_utils/analyse_utils.py (calculate_metrics :628-728, calculate_prediction_entropy :294-310) and ui.py:55-59 (BLOSUM62
 * similarity), in one pass over the prediction matrix on the GPU.  Residues are indices 0..19 in the order ACDEFGHIKLMNPQRSTVWY.
 * matrix: host [n, k] of TH_F16 or TH_F32, 1 <= k <= 1024; col_res: host int8[k], the residue that owns each column (the identity
 * for k = 20, the rotamer codec's owner for k = 338; any order); true_res: host int8[n], 0..19 or -1 (unlabelled).  Per row:
 *   pred_out[i]    = col_res[argmax_i] under th_argmax_letters' rules (first maximum, first NaN) — the FASTA letter;
 *   rank_out[i]    = rank of the true residue t: with s_r = max of residue r's columns and c_r the first column reaching it,
 *                    #{r : s_r > s_t or (s_r == s_t and c_r < c_t)}; 20 ("never a hit") when t owns no column; a row holding a NaN
 *                    or an infinity ranks 0 if pred == t, else 20; -1 for an unlabelled row;
 *   entropy_out[i] = Shannon entropy in bits of the row normalised by its sum (scipy.stats.entropy(row, base=2)), float64; NaN when
 *                    the sum is 0 or the row holds a NaN, an infinity or a negative value (scipy gives -inf for the last).
 * Each output may be NULL.  Totals over the whole matrix (labelled rows only, but n_nonfinite counts every row) are 64-bit integers,
 * independent of arrival order: two calls give the same bytes.  similar = BLOSUM62(true, pred) > 0.  The host rows are staged to
 * `device` in blocks of up to 262 144 rows (at most 256 MB; TH_ANALYSIS_BLOCK_ROWS overrides the row count, results unchanged),
 * copies overlapping the kernel of the previous block.  TH_EINVAL: dtype, k, or a col_res / true_res value out of range.  n = 0
 * returns zero totals. */
typedef struct th_analysis_totals {
    int64_t confusion[20][20];    /* [true][predicted]                               */
    int64_t rank_hist[21];        /* rank of the true residue; bucket 20: never a hit */
    int64_t n_labelled, n_nonfinite, n_similar;
} th_analysis_totals;
int th_analyse_probs(int device, const void* matrix, int dtype, int64_t n, int64_t k, const int8_t* col_res, const int8_t* true_res,
                     int8_t* pred_out, int8_t* rank_out, double* entropy_out, th_analysis_totals* totals);

/* ---- per-class evaluation: analyse_rotamers.py / predict.py --output_auc — what the reference's calculate_rotamer_metrics
 * (design_utils/analyse_utils.py:731-898) computes with sklearn for a 338-class rotamer model: k x k confusion, top-k over the k
 * columns, and the integer table behind the ROC AUC one-vs-one and one-vs-rest.  matrix: host [n, k] of TH_F16 or TH_F32,
 * 1 <= k <= 1024, n < 2^31; true_class: host int16[n], 0..k-1 or -1 (unlabelled).  A row is SCORED when it is labelled and holds
 * no NaN and no infinity.  Per row:
 *   pred_out[i] = arg-max under th_argmax_letters' rules (first maximum, first NaN);
 *   rank_out[i] = #{c : x_c > x_t or (x_c == x_t and c < t)} for the true class t; a row holding a NaN or an infinity ranks 0 if
 *                 pred == t, else k; -1 for an unlabelled row.
 * Totals (all int64, independent of grid, staging blocks and arrival order — two calls give the same bytes):
 *   confusion[t * k + p]   labelled rows of true class t predicted as p;
 *   rank_hist[r]           labelled rows by rank_out; bucket k: a non-finite row that was missed;
 *   scored_count[c]        n_c, the scored rows of class c;
 *   pair_u2[a * k + b]     U2[a][b] = sum over scored rows i of class a and j of class b of 2 [x[i][a] > x[j][a]] + [x[i][a] == x[j][a]]
 *                          (twice the Mann-Whitney statistic of column a, ties half; numeric comparison of the stored values,
 *                          -0 == +0; U2[a][a] = 0).  auc(a|b) = U2[a][b] / (2 n_a n_b).  NULL skips the AUC sweep: the other
 *                          outputs are the same bytes either way;
 *   counts                 labelled rows, rows holding a NaN or an infinity (labelled or not), scored rows.
 * The matrix is staged in the blocks of th_analyse_probs (TH_ANALYSIS_BLOCK_ROWS overrides the row count, results unchanged); the
 * AUC sweep is a second pass that re-stages the blocks unless the whole matrix is one block, which stays resident.  Device memory
 * beside the two staging slots: 8 k^2 (+ 8 k^2 with pair_u2) bytes of totals and, with pair_u2, 21 bytes per row plus the sort's
 * scratch.  TH_EINVAL: NULL totals, dtype, k, n, or a label outside -1..k-1.  n = 0 returns zero totals. */
typedef struct th_class_counts { int64_t n_labelled, n_nonfinite, n_scored; } th_class_counts;
int th_analyse_classes(int device, const void* matrix, int dtype, int64_t n, int64_t k, const int16_t* true_class,
                       int16_t* pred_out, int16_t* rank_out,           /* [n] each, may be NULL                       */
                       int64_t* confusion,                             /* [k*k], [true][predicted], labelled rows     */
                       int64_t* rank_hist,                             /* [k+1], bucket k: non-finite row, missed     */
                       int64_t* scored_count,                          /* [k]   n_c                                   */
                       int64_t* pair_u2,                               /* [k*k] U2[a][b]; NULL: skip the AUC sweep    */
                       th_class_counts* counts);

/* ---- structure properties: analyse_properties.py — the packing density of the reference's design_utils/analyse_utils.py
 * (tag_packing_density :44-86: the atomic contact number of Weiss 2007; _extract_packdensity_from_polypeptide :149-201: its
 * per-residue summary), for a BATCH of structures in one submission.  The reference loops over the atoms of one structure in
 * NumPy, O(N^2) float64 per structure.  All arrays are host memory.
 *   device        HIP device index;
 *   xyz           double[total][3], the atoms of all structures, structure after structure (Angstrom; any value, NaN and
 *                 infinities included);
 *   total         number of atoms, 0 <= total <= 2^31 - 257;
 *   offsets       int64[n_structures + 1]: structure s owns atoms offsets[s] .. offsets[s + 1]; offsets[0] = 0, non-decreasing,
 *                 offsets[n_structures] = total.  Pairs are formed within a structure only; a structure may be empty;
 *   radius        any double;
 *   group         int32[total]: the residue (0 .. n_groups - 1, an index within the batch) that atom i is reported under, or -1
 *                 for an atom that is only a neighbour.  The atoms of one residue are consecutive.  Read only when n_groups > 0;
 *   selected      uint8[total]: non-zero where the atom enters its residue's value.  Read only when n_groups > 0;
 *   n_groups      number of residues, 0 <= n_groups <= 2^31 - 1;
 *   density_out   int32[total] or NULL (the per-atom counts are then not copied back):
 *                   density[i] = #{ j in the structure of i, j == i included : sqrt((dx*dx + dy*dy) + dz*dz) < radius } - 1
 *                 with dx = x_j - x_i ..., evaluated in float64 in exactly this order, every product and sum rounded on its own (no
 *                 fused multiply-add), the root correctly rounded: NumPy's np.sqrt(np.square(xyz - xyz[i]).sum(axis=1)) < radius,
 *                 bit for bit, pairs at a distance of "exactly" the radius included.  Hence: the atom counts itself and 1 is
 *                 subtracted, so an atom with a NaN or infinite coordinate gets -1; atoms at equal coordinates count each other;
 *                 radius <= 0 or NaN gives -1 everywhere.  (The kernel compares the squared distance with th_packing_threshold(radius).)
 *   residue_out   double[n_groups] (required when n_groups > 0): the reference's running value over the SELECTED atoms of the
 *                 residue in index order:  cur = -1;  for each: cur = (cur == -1) ? density : (cur + density) / 2.  It is not the
 *                 mean and the order matters; -1.0 for a residue without a selected atom; like the reference, a leading selected atom
 *                 whose density is -1 is indistinguishable from "none yet" and is replaced by the next;
 *   kernel_ms_out NULL, or receives the device time of the two kernels (events around them), in milliseconds.
 * Integers and exact halves of small integers only: independent of grid and arrival order, two calls give the same bytes.
 * Device memory: 28 bytes per atom + 12 per 256 atoms of every structure (+ 1 per atom and 16 per residue with n_groups > 0).
 * TH_EINVAL, before anything is launched or written: a NULL that is required, a negative size, total or n_groups above the limit,
 * offsets not as described, a group value outside -1 .. n_groups - 1, a residue whose atoms are not consecutive.  total = 0
 * (n_structures = 0, or only empty structures) returns without launching: residue_out is all -1.0. */
int th_packing_density(int device, const double* xyz, int64_t total, const int64_t* offsets, int64_t n_structures, double radius,
                       const int32_t* group, const uint8_t* selected, int64_t n_groups, int32_t* density_out, double* residue_out,
                       double* kernel_ms_out);
/* T(radius): the smallest double whose correctly rounded square root is >= radius, so that  sqrt(s) < radius  <=>  s < T  for every
 * double s >= +0, infinite or NaN.  Not radius * radius in general.  0 for radius <= 0, radius itself when it is NaN or +infinity.
 * Host code. */
double th_packing_threshold(double radius);

/* ---- rotamer labels from structures: analyse_rotamers.py / tag_rotamers.py — what the reference's tag_pdb_with_rot and
 * extract_rotamer_encoding (design_utils/analyse_utils.py:901-1036) get from ampal's tag_sidechain_dihedrals: the chi angles of every
 * residue and its class among the 338 categories of get_rotamer_codec, for a BATCH of structures in one submission.
 *
 *     *** PARITY UNPINNED AGAINST AMPAL ***  ampal is neither in the reference tree nor installed where this project is built.  The
 *     rule below — atom paths, bin edges, the ALA / GLY class — is this project's reading of ampal 1.5's
 *     classify_angle_as_rotamer / tag_sidechain_dihedrals, and no test can pin it against ampal itself.
 *
 * All arrays are host memory.
 *   xyz           double[total][3], atoms in file order (any value);
 *   atom_name     uint32[total]: the stripped atom name as 4 ASCII bytes, left-justified, zero-padded, little-endian ("CA" = 0x4143);
 *   total         number of atoms, 0 <= total <= 2^31 - 1;
 *   res_offsets   int64[n_res + 1], non-decreasing, within 0 .. total: residue r owns atoms res_offsets[r] .. res_offsets[r + 1]
 *                 (atoms outside every residue are allowed and never read);
 *   res_type      int8[n_res]: 0..19 in the order of design_utils.amino_acids.standard_amino_acids (ALA CYS ASP GLU PHE GLY HIS ILE
 *                 LYS LEU MET ASN PRO GLN ARG SER THR VAL TRP TYR: the codec's order), or -1 for anything else;
 *   n_res         0 <= n_res <= 2^31 - 1;
 *   flags         bit 0: ALA and GLY get -1 instead of their single class;
 *   cls_out       int16[n_res]: the index into get_rotamer_codec()[1], or -1 (unlabelled);
 *   chi_out       double[n_res][4] or NULL: degrees in (-180, 180], NaN where the residue has no such angle or is unlabelled;
 *   kernel_ms     NULL, or receives the device time of the kernel (events around it), in milliseconds.
 * Every chi angle is a window of four consecutive atoms on one path of n_chi + 3 atoms, N CA CB + the residue's tail
 * (th_rotamer_table; ARG: CG CD NE CZ, ASN ASP: CG OD1, CYS: SG, GLN GLU: CG CD OE1, HIS: CG ND1, ILE: CG1 CD1, LEU PHE TRP TYR: CG CD1,
 * LYS: CG CD CE NZ, MET: CG SD CE, PRO: CG CD, SER: OG, THR: OG1, VAL: CG1; ALA and GLY have none): chi k uses path[k .. k + 3].  Each
 * name is searched among the residue's own atoms on the device; the first atom with the name wins.  With a, b, c, d the four atoms:
 *   b1 = b - a, b2 = c - b, b3 = d - c, n1 = b1 x b2, n2 = b2 x b3, chi = atan2(|b2| (b1 . n2), n1 . n2) in degrees (IUPAC sign),
 * in float64, every product and sum rounded on its own, dot products summed as (x + y) + z.  Bin 1: 0 <= chi < 120; bin 3:
 * -120 <= chi < 0; bin 2 (trans): everything else.  class = class_base[type] + sum_k (bin_k - 1) 3^(n_chi - 1 - k): the first angle
 * varies slowest, as itertools.product orders the codec.  UNLABELLED (-1, chi all NaN): res_type -1, any path atom absent, any angle
 * not finite.  ALA and GLY carry their single class ALA_0 / GLY_0 whatever their atoms (flags bit 0: -1).
 * Integers decided by float64 comparisons: independent of grid and arrival order, two calls give the same bytes.  Device memory:
 * 28 bytes per atom + 11 (43 with chi_out) per residue.  TH_EINVAL, before anything is launched or written: a negative or too large
 * size, a NULL that is required, res_offsets decreasing or outside 0 .. total, a res_type outside -1 .. 19.  n_res = 0 is success. */
int th_tag_rotamers(int device, const double* xyz, const uint32_t* atom_name, int64_t total, const int64_t* res_offsets,
                    const int8_t* res_type, int64_t n_res, int flags, int16_t* cls_out, double* chi_out, double* kernel_ms);
/* The table th_tag_rotamers uses, for one residue type 0..19: the number of chi angles, the index of the type's first class, and the
 * n_chi + 3 path names (zero-padded to 4 bytes, not terminated when 4 long; all zero beyond the path and for ALA / GLY).  Any output
 * may be NULL.  Host code. */
int th_rotamer_table(int res_type, int* n_chi, int* class_base, char names[7][4]);

/* ---- *** PARITY UNPINNED AGAINST SCWRL4 *** side chains from rotamer classes: build_sidechains.py — the inverse of th_tag_rotamers.
 * From N, CA, C, a residue type and chi angles per residue to every side-chain heavy atom, for a BATCH of structures in one
 * submission; then the deviation from native atoms of the same name, and the steric clashes of the result.  The reference gets
 * side chains from SCWRL4 (analyse_rotamers.py analyses 2 and 3, pack_sidechains), which searches rotamers by energy; here the
 * rotamer is the caller's choice (a predicted class, the native angles) and nothing is searched.
 *
 *     *** PARITY UNPINNED AGAINST SCWRL4 ***  SCWRL4 is not available where this project is built.  The tree of internal
 *     coordinates (csrc/sidechain_table.h; th_sidechain_table), its values (standard stereochemistry after Engh & Huber 1991, the
 *     offsets of the sp3 branches from the means of 1ubq) and the rules below are this project's own; no test can pin them against
 *     SCWRL4 itself.  Rebuilding 1ubq from its native chi angles gives 0.347 Angstrom RMSD over its 297 side-chain heavy atoms.
 *
 * All arrays are host memory.
 *   backbone            double[n_res][nb][3] with nb = 3 (N, CA, C) or, with TH_SC_BACKBONE_O in flags, nb = 4 (N, CA, C, O).  Any
 *                       value; O is used by the clash count alone and may be NaN;
 *   res_type            int8[n_res]: 0..19 in the codec's order (th_tag_rotamers), -1 for anything else: the type that is BUILT;
 *   chi                 double[n_res][4], degrees; only the angles the type needs are read (th_rotamer_table's n_chi);
 *   chain_id            NULL (one chain) or int32[n_res]: any labels; read by the clash count alone;
 *   struct_offsets      int64[n_struct + 1]: structure s owns residues struct_offsets[s] .. struct_offsets[s + 1]; starts at 0,
 *                       non-decreasing, ends at n_res.  A structure may be empty;
 *   n_struct, n_res     0 <= n_struct <= 2^31 - 1, 0 <= n_res <= TH_SC_MAX_RESIDUES;
 *   native_xyz, native_name, native_total, native_res_offsets
 *                       the native atoms in the format of th_tag_rotamers (packed names; residue r owns atoms
 *                       native_res_offsets[r] .. [r + 1], non-decreasing, within 0 .. native_total), and
 *   native_type         int8[n_res], the native residue types, -1..19.  native_res_offsets NULL: no native; the other four and
 *                       out_n_matched, out_sum_sq must then be NULL / 0;
 *   clash_distance      finite and > 0 when a clash output is asked for (the Python layer's default: 2.5 Angstrom);
 *   flags               TH_SC_BACKBONE_O or 0;
 *   out_xyz             double[n_res][10][3]: the atoms of residue r in the order of th_sidechain_table, NaN beyond n_built;
 *   out_n_built         int32[n_res]: the number of atoms of the type, or 0;
 *   out_n_matched       int32[n_res], out_sum_sq double[n_res] (both required with a native, NULL without);
 *   out_clashes         int32[n_res] or NULL;  out_struct_pairs  int64[n_struct] or NULL.  Both NULL: no clash kernel runs;
 *   kernel_ms           NULL, or receives the device time of the kernels (events around them), in milliseconds.
 * BUILDING.  Atom d with parents a, b, c (N, CA, C or earlier atoms of the residue), bond length L, bond angle t = b-c-d and
 * dihedral p = a-b-c-d = chi[k] + offset (the offset alone for k = -1), all float64, every product and sum rounded on its own:
 *   bc = (c - b) / |c - b|,  n = (b - a) x bc divided by its length,  m = n x bc,
 *   d = c + ((-(L cos t)) bc + ((L sin t) cos p) m) + ((L sin t) sin p) n,      angles in radians = degrees * (pi / 180).
 * The dihedral of the built atoms, measured by th_tag_rotamers' formula, is p.  CB is built like any other atom, on (C, N, CA).
 * UNBUILT (all ten atoms NaN, n_built = 0, no match, no clash): res_type -1 or GLY; a coordinate of N, CA or C that is not finite;
 * a chi angle the type needs that is not finite; any atom that comes out not finite (N, CA, C on a line: 0 / 0 in n).  Never an
 * error, and the residues beside it are not affected.
 * DEVIATION.  Where native_type[r] == res_type[r] and r is built, every built atom takes the FIRST native atom of residue r with
 * its name (a native atom with a coordinate that is not finite matches nothing): n_matched counts them, sum_sq is the sum of
 * (dx*dx + dy*dy) + dz*dz in table order.  The caller forms sqrt(sum_sq / n_matched).  NO SYMMETRY CORRECTION: a PHE / TYR ring or
 * an ASP / GLU carboxylate deposited with its two equivalent atoms the other way round (chi2 off by 180 degrees) is reported as it
 * is named, and so is an ASN / GLN / HIS flip.
 * CLASHES.  The atoms of a structure are the built side-chain atoms and the nb backbone atoms of every residue (those of unbuilt
 * residues too).  A pair CLASHES when sqrt((dx*dx + dy*dy) + dz*dz) < clash_distance (strict; the kernel compares the squared
 * distance with th_packing_threshold(clash_distance), the same decision for every double).  Counted are pairs of a side-chain atom
 * of residue i with an atom of residue j != i of the same structure, except: between chain neighbours — |i - j| = 1, indices in
 * the structure, and chain_id[i] == chain_id[j] — only side chain against side chain (the bonded backbone is no clash); two
 * consecutive residues of DIFFERENT chains are counted in full; a pair of two SG atoms is never counted (a disulfide).
 * clashes[r] is the number of counted pairs whose side-chain atom is of r (a side chain - side chain pair counts for both
 * residues); pairs[s] is the number of unordered counted pairs of structure s, each once.
 * No atomics.  A residue's atoms depend on its own inputs, a structure's counts on its own residues alone — not on the place in
 * the batch — and two calls give the same bytes.  Device memory: about 400 bytes per residue + 28 per native atom.  TH_EINVAL,
 * before anything is launched or written: a negative or too large size, a NULL that is required, struct_offsets that decrease, do
 * not start at 0 or do not end at n_res, native_res_offsets decreasing or outside 0 .. native_total, a type outside -1 .. 19,
 * unknown flag bits, native arrays or outputs without native_res_offsets, a clash output with a clash_distance that is not finite
 * or not > 0.  n_res = 0 is success without a launch (pairs all 0). */
#define TH_SC_BACKBONE_O 1
#define TH_SC_MAX_RESIDUES 134217727 /* (2^31 - 1) / 16 */
int th_build_sidechains(int device, const double* backbone, const int8_t* res_type, const double* chi, const int32_t* chain_id,
                        const int64_t* struct_offsets, int64_t n_struct, int64_t n_res, const double* native_xyz,
                        const uint32_t* native_name, int64_t native_total, const int64_t* native_res_offsets, const int8_t* native_type,
                        double clash_distance, int flags, double* out_xyz, int32_t* out_n_built, int32_t* out_n_matched,
                        double* out_sum_sq, int32_t* out_clashes, int64_t* out_struct_pairs, double* kernel_ms);
/* The table th_build_sidechains uses, for one residue type 0..19: the number of side-chain heavy atoms (0 for GLY) and, per atom in
 * build order, its name (zero-padded to 4 bytes), its three parents a, b, c (0 = N, 1 = CA, 2 = C, 3 + j = atom j of this list),
 * the chi index k (-1: none) and {bond length |cd| in Angstrom, bond angle b-c-d, dihedral offset} in degrees; then the bonds that
 * close the type's rings, which the tree does not use: their two atoms (indices into this list; -1 beyond n_closure) and the
 * length the table states for each.  Rows beyond n_atoms are zero (chi_index -1).  Any output may be NULL.  Host code. */
int th_sidechain_table(int res_type, int* n_atoms, char names[10][4], int8_t parents[10][3], int8_t chi_index[10],
                       double geometry[10][3], int* n_closure, int8_t closure_atoms[2][2], double closure_length[2]);

/* ---- *** PARITY UNPINNED AGAINST SCWRL4 *** side chains packed by a rotamer search: pack_sidechains.py, analyse_rotamers.py --pack.
 * th_build_sidechains builds the class the caller chose; this CHOOSES, for a BATCH of structures in one submission: for every
 * residue one of the 3^n_chi classes of its type, under a steric ladder and optionally a rotamer model's own probabilities, by
 * greedy sweeps from a deterministic start.  It returns classes and energies only; the atoms, the RMSD and the clash counts of the
 * result come from th_build_sidechains on the chosen classes.
 *
 *     *** PARITY UNPINNED AGAINST SCWRL4 ***  The reference hands a sequence and a backbone to SCWRL4 (analyse_rotamers.py analyses
 *     2 and 3), which is not available where this project is built.  The rule below is this project's own.  It is not SCWRL4's
 *     backbone-dependent rotamer library nor its energy, it knows no hydrogen bonds, and it finds a local minimum, not the global
 *     one; no test can pin it against SCWRL4 itself.
 *
 * All arrays are host memory.  backbone, res_type, chain_id, struct_offsets, n_struct, flags as in th_build_sidechains
 * (n_res <= TH_PACK_MAX_RESIDUES); res_type is the type to build.
 *   ladder, n_levels    double[n_levels], 1 <= n_levels <= TH_PACK_MAX_LEVELS: finite, positive, strictly increasing distances in
 *                       Angstrom (the Python layer's default: 2.0, 2.5, 3.0, 3.5);
 *   prior_cost          NULL (none) or int32[n_res][81]: the cost of candidate k of residue r, 0 .. TH_PACK_MAX_COST; entries beyond
 *                       the type's candidates are ignored (timed_hip.packer.prior_costs: round(-1000 log2 p), computed on the host);
 *   clash_weight        1 .. TH_PACK_MAX_COST: the cost of one ladder level (the Python layer's default: 2000);
 *   max_sweeps          0 .. TH_PACK_MAX_SWEEPS;
 *   out_cls             int16[n_res]: the chosen class (an index into the 338 of th_tag_rotamers) or -1;
 *   out_cost_initial, out_cost_final      int64[n_res]: the residue's cost in the initial and in the final state, 0 without a class;
 *   out_energy_initial, out_energy_final  int64[n_struct];
 *   out_search          int32[n_struct][4]: sweeps run, moves made, converged (0 / 1), status (TH_PACK_OK, TH_PACK_TOO_LONG);
 *   kernel_ms           NULL or double[3]: the device time of the candidates, the backbone and the search kernel, in milliseconds.
 * CANDIDATES.  Residue r of type 0..19 has the 3^n_chi classes of its type as candidates, in class order: candidate k is class
 * th_rotamer_table's class_base + k with every chi at its bin centre — 60 / 180 / -60 degrees for bins 1 / 2 / 3, the first angle
 * varying slowest — and its atoms are placed exactly as th_build_sidechains places them (the same table, the same float64
 * operations in the same order).  ALA has one candidate, CB alone.  GLY and type -1 have none: their backbone stays in the energy
 * and they get class -1.  A residue whose N, CA or C is not finite has no candidates; a candidate with an atom that comes out not
 * finite is excluded.
 * PENALTY of a pair of atoms: the number of ladder levels t with sqrt((dx*dx + dy*dy) + dz*dz) < ladder[t], decided as
 * th_build_sidechains decides a clash: the squared distance against th_packing_threshold(ladder[t]), false for NaN.
 * PAIRS that count: the CLASHES rule of th_build_sidechains, unchanged — a side-chain atom of i against any atom (the nb backbone
 * atoms, the current side-chain atoms) of a residue j != i of the same structure; between chain neighbours (|i - j| = 1 and equal
 * chain_id) side chain against side chain only; SG-SG never.
 * COST of candidate k of residue i given the current choice of all others, int64:
 *   cost = prior_cost[i][k] + clash_weight * (penalty against all backbone atoms + penalty against the current side-chain atoms of
 *   every other residue).
 * ENERGY of a structure = sum of the priors of the chosen candidates + clash_weight * (all side chain - backbone penalties + every
 * side chain - side chain pair once).
 * SEARCH.  Initial state: for every residue the candidate of lowest prior + clash_weight * backbone penalty, the lowest k on ties.
 * Then sweeps over the residues of the structure in index order: residue i moves to its candidate of lowest cost (lowest k on
 * ties) only if that cost is strictly below the cost of its current candidate.  The energy is an integer and falls with every
 * move, so the search ends.  It stops after a sweep without a move (converged = 1) or after max_sweeps sweeps; max_sweeps = 0
 * returns the initial state.  A structure in which no residue has two candidates cannot move: no sweep is run and converged = 1.
 * A structure of more than TH_PACK_MAX_STRUCT_RESIDUES residues is not packed: status TH_PACK_TOO_LONG, class -1 everywhere,
 * everything else 0 — and the structures beside it are packed.  (One workgroup searches one structure, serially over its
 * residues; the limit bounds its run time, not its memory.)
 * Everything the search decides is an integer; no atomics; no pair is culled; a structure's outputs depend on its own residues
 * alone, not on its place in the batch, and two calls give the same bytes.  Device memory: about 250 bytes per candidate + 380
 * (+ 324 with a prior) per residue.  TH_EINVAL, before anything is launched or written: a negative or too large size, a NULL that
 * is required (every output, ladder, and with residues backbone and res_type), struct_offsets not as described, a type outside
 * -1 .. 19, a ladder that is not 1..8 finite positive strictly increasing levels, clash_weight, max_sweeps or a read entry of
 * prior_cost out of range, unknown flag bits.  n_struct = 0 is success without a launch. */
#define TH_PACK_MAX_CANDIDATES 81
#define TH_PACK_MAX_LEVELS 8
#define TH_PACK_MAX_COST 1000000
#define TH_PACK_MAX_SWEEPS 1000
#define TH_PACK_MAX_STRUCT_RESIDUES 4096
#define TH_PACK_MAX_RESIDUES 16777216 /* 2^24: at most 81 x 2^24 < 2^31 candidates */
#define TH_PACK_OK 0
#define TH_PACK_TOO_LONG 1
int th_pack_sidechains(int device, const double* backbone, const int8_t* res_type, const int32_t* chain_id, const int64_t* struct_offsets,
                       int64_t n_struct, int64_t n_res, const double* ladder, int n_levels, const int32_t* prior_cost,
                       int32_t clash_weight, int32_t max_sweeps, int flags, int16_t* out_cls, int64_t* out_cost_initial,
                       int64_t* out_cost_final, int64_t* out_energy_initial, int64_t* out_energy_final, int32_t* out_search,
                       double* kernel_ms);

/* ---- superposition of models on their native: analyse_models.py — what the reference's calculate_RMSD_and_gdt
 * (scripts/analyse_af2.py) gets from PyMOL one pair at a time: cmd.align on the CA atoms, its RMSD, and the fractions of aligned
 * pairs within 1, 2, 4 and 8 Angstrom.  Here for a BATCH of position-paired coordinate lists in one launch.
 *
 *     *** PARITY UNPINNED AGAINST PYMOL ***  PyMOL is not available where this project is built.  The rule below is this project's
 *     reading of the DOCUMENTED behaviour of cmd.align (cycles default 5, cutoff default 2.0: "outlier rejection cutoff in RMS") on
 *     atoms that are already paired by position; it is not PyMOL's code, it aligns no sequences, and no test can pin it against
 *     PyMOL itself.
 *
 * All arrays are host memory.
 *   ref_xyz, mob_xyz   double[total][3]: the reference (target) and the mobile coordinates of all pairs, pair after pair; position i
 *                      of one list is paired with position i of the other (any value, NaN and infinities included);
 *   total              number of positions, 0 <= total <= 2^31 - 1;
 *   offsets            int64[n_pairs + 1]: pair p owns positions offsets[p] .. offsets[p + 1] of both lists; offsets[0] = 0,
 *                      non-decreasing, offsets[n_pairs] = total.  A pair may be empty;
 *   n_pairs            0 <= n_pairs <= 2^31 - 1;
 *   cycles             refinement cycles at most, >= 0 (PyMOL's default: 5);
 *   cutoff             outlier rejection in units of the RMS, finite and > 0 (PyMOL's default: 2.0);
 *   dist_out           double[total]: d_i under the final fit, NaN at an invalid position;
 *   kept_out           uint8[total]: 1 where the position is in the final kept set;
 *   rmsd_out           double[n_pairs][3]: rmsd_kept, rmsd_all, rmsd_fit_all;
 *   count_out          int32[n_pairs][7]: n_valid, n_kept, cycles_run, then the number of valid positions with d_i <= 1, 2, 4, 8;
 *   transform_out      double[n_pairs][12] or NULL: rows of [R | t], moved = R mob + t with t = cr - R cm (the identity when no
 *                      position is valid);
 *   kernel_ms          NULL, or receives the device time of the kernel (events around it), in milliseconds.
 * The rule, for one pair of equally long lists ref[i], mob[i], all arithmetic float64:
 *   - a position is VALID when all six coordinates are finite.  An invalid position is never kept, its d_i is NaN and it counts in
 *     no total;
 *   - FIT over a kept set: the centroids cm, cr are plain sums over the kept positions in index order, divided by the count (the
 *     kernel sums each lane's positions l, l + 64, ... in index order and then the 64 lanes in a fixed tree).  The 3 x 3
 *     cross-covariance S[x][y] = sum (mob - cm)_x (ref - cr)_y is taken over the centred coordinates: two passes, never
 *     sum xy - n mean(x) mean(y).  The rotation is the PROPER one (determinant +1) that minimises the squared deviation, from Horn's
 *     symmetric 4 x 4 matrix
 *         [ Sxx+Syy+Szz   Syz-Szy       Szx-Sxz       Sxy-Syx     ]
 *         [ Syz-Szy       Sxx-Syy-Szz   Sxy+Syx       Szx+Sxz     ]
 *         [ Szx-Sxz       Sxy+Syx      -Sxx+Syy-Szz   Syz+Szy     ]
 *         [ Sxy-Syx       Szx+Sxz       Syz+Szy      -Sxx-Syy+Szz ]
 *     whose unit eigenvector of largest eigenvalue (cyclic Jacobi, pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), at most 10 sweeps; of
 *     equal eigenvalues the first) is the quaternion (w, x, y, z) of R.  A mirror image therefore gives a large RMSD, not zero;
 *   - moved_i = R (mob_i - cm) + cr for every valid position, and d_i = |moved_i - ref_i|, the square root of a sum of three
 *     squares, computed as such (not through the eigenvalue);
 *   - cycle 0 keeps every valid position.  REFINEMENT, at most `cycles` times: rms = sqrt(sum over kept of d_i^2 / n_kept); the kept
 *     positions with d_i > cutoff * rms are dropped and the fit is made again over the smaller set — unless none is dropped or
 *     fewer than 3 would remain: the set then stays as it is and refinement ends.  cycles_run counts the fits made after cycle 0;
 *   - rmsd_kept: over the final kept set under the final fit (the number cmd.align returns); rmsd_all: over all valid positions
 *     under the final fit; rmsd_fit_all: the value of cycle 0, the conventional RMSD of the whole set.  The counts within 1, 2, 4 and
 *     8 Angstrom are over all valid positions under the final fit; the GDT fractions and their mean are formed by the caller;
 *   - n_valid = 0: the three RMSDs are NaN and all counts 0.  n_valid = 1 or 2: the fit is made (its RMSD is the unique minimum, its
 *     rotation need not be unique) and there is no refinement.
 * One launch for the whole batch, the refinement loop inside the kernel; no atomics.  A pair's outputs depend on its own coordinates
 * alone — not on its place in the batch or on its neighbours — and two calls give the same bytes.  Device memory: 57 bytes per
 * position + 60 (156 with transform_out) per pair.  TH_EINVAL, before anything is launched or written: a negative or too large size,
 * a NULL that is required (offsets, rmsd_out, count_out; with total > 0 also both lists, dist_out and kept_out), offsets that
 * decrease, do not start at 0 or do not end at total, cycles < 0, cutoff not finite or <= 0.  n_pairs = 0 (with total = 0) is
 * success without a launch. */
int th_superpose(int device, const double* ref_xyz, const double* mob_xyz, int64_t total, const int64_t* offsets, int64_t n_pairs,
                 int cycles, double cutoff, double* dist_out, uint8_t* kept_out, double* rmsd_out, int32_t* count_out,
                 double* transform_out, double* kernel_ms);

/* ---- *** PARITY UNPINNED AGAINST OPENSTRUCTURE *** lDDT of models against their native: analyse_models.py --lddt — the local
 * Distance Difference Test (Mariani et al. 2013), the measured counterpart of the pLDDT that AlphaFold2 writes into the B-factor
 * column of its models (the reference plots that prediction in plot_af2IDDT_vs_position).  Here for a BATCH of position-paired
 * coordinate lists in one launch.
 *
 *     *** PARITY UNPINNED AGAINST OPENSTRUCTURE ***  Neither OpenStructure nor AlphaFold's lddt.py is available where this project
 *     is built.  The rule below is this project's reading of the PUBLISHED definition (Mariani et al. 2013) in the CA-only form
 *     AlphaFold uses: one position per residue, no stereochemistry checks, strict inequalities on both tests; it is neither
 *     implementation's code, it aligns no sequences, and no test can pin it against OpenStructure itself.
 *
 * All arrays are host memory.
 *   ref_xyz, mob_xyz   double[total][3]: the reference (native) and the model coordinates of all pairs, pair after pair; position i
 *                      of one list is paired with position i of the other (any value, NaN and infinities included);
 *   total              number of positions, 0 <= total <= 2^31 - 1;
 *   offsets            int64[n_pairs + 1]: pair p owns positions offsets[p] .. offsets[p + 1] of both lists; offsets[0] = 0,
 *                      non-decreasing, offsets[n_pairs] = total.  A pair may be empty;
 *   n_pairs            0 <= n_pairs <= 2^31 - 1;
 *   radius             inclusion radius, finite and > 0 (the published default: 15.0);
 *   thresholds         double[4], each finite and > 0 (the published default: 0.5, 1, 2, 4);
 *   residue_out        int32[total][5]: n_i, c_i[0..3]; five zeros at an invalid position;
 *   pair_out           int64[n_pairs][6]: n_valid, N, C[0..3];
 *   kernel_ms          NULL, or receives the device time of the two kernels (events around them), in milliseconds.
 * The rule, for one pair of equally long lists ref[i], mob[i], all arithmetic float64 and no fused multiply-add:
 *   - a position is VALID when all six of its coordinates are finite.  An invalid position is never an i and never a j: an infinity
 *     in one list does not leak through the other list's distance (the kernel makes both lists NaN at such a position);
 *   - DISTANCE  d(a, b) = sqrt((dx*dx + dy*dy) + dz*dz), in that order, each product and sum rounded on its own, the square root
 *     correctly rounded;
 *   - an ordered pair (i, j) is INCLUDED when j != i, both positions are valid and d_ref(i, j) < radius.  Strict.  Two different
 *     positions with identical coordinates are a pair like any other.  (The kernel compares the squared distance with
 *     th_packing_threshold(radius), which decides the same for every double, and takes square roots of included pairs only.)
 *   - an included pair is PRESERVED at threshold t when |d_ref(i, j) - d_mob(i, j)| < t.  Strict;
 *   - per position: n_i is the number of included j, c_i[k] the number of those preserved at thresholds[k];
 *   - per pair: n_valid, N = sum n_i and C[k] = sum c_i[k], over ORDERED pairs (every unordered pair counts twice), 64-bit;
 *   - the caller forms the fractions, as it does for GDT: lddt_i = sum_k c_i[k] / (4 n_i), NaN when n_i = 0, and
 *     lddt = sum_k C[k] / (4 N), NaN when N = 0.  The global score is PAIR-weighted, as in both published implementations; it is
 *     not the mean of lddt_i.
 * MIRROR IMAGES: every distance of a mirror image is that of the original, so lDDT does not see one — the mirror case of the
 * superposition fixture scores 1.0 here where th_superpose reports 10.7 Angstrom.  Conversely one re-oriented domain costs
 * th_superpose everything and lDDT only the pairs across the hinge.  That is the reason to report both.  (th_tmscore, below,
 * superposes with a proper rotation and scores that mirror image 0.308.)
 * All outputs are integers decided by float64 comparisons: a pair's outputs depend on its own coordinates alone — not on its place
 * in the batch or on its neighbours — and two calls give the same bytes.  No atomics.  Device memory: 68 bytes per position + 8 per
 * 256 positions of every pair + 56 per pair; the O(L^2) distances exist in registers only.  TH_EINVAL, before anything is launched
 * or written: a negative or too large size, a NULL that is required (offsets, thresholds, pair_out; with total > 0 also both lists
 * and residue_out), offsets that decrease, do not start at 0 or do not end at total, a radius or a threshold that is not finite
 * or not > 0.  n_pairs = 0 (with total = 0) is success without a launch. */
int th_lddt(int device, const double* ref_xyz, const double* mob_xyz, int64_t total, const int64_t* offsets, int64_t n_pairs,
            double radius, const double* thresholds, int32_t* residue_out, int64_t* pair_out, double* kernel_ms);

/* ---- *** PARITY UNPINNED AGAINST OPENSTRUCTURE *** All-atom lDDT with symmetric side chains: analyse_models.py --lddt_all_atom,
 * build_sidechains.py --lddt, pack_sidechains.py --lddt — the local Distance Difference Test (Mariani et al. 2013) over the heavy
 * atoms of a model against those of its native, the form CASP, CAMEO and OpenStructure quote, and the superposition-free measure of
 * side-chain placement: the names of chemically equivalent atoms (the ring edges of PHE and TYR, the carboxylate oxygens of ASP and
 * GLU, ...) are resolved per residue before anything is counted.  Here for a BATCH of atom-paired coordinate lists.
 *
 *     *** PARITY UNPINNED AGAINST OPENSTRUCTURE ***  OpenStructure is not available where this project is built.  The rule below is
 *     this project's reading of the PUBLISHED definition (Mariani et al. 2013) in float64 with fp contract(off): no stereochemistry
 *     checks, no sequence-separation filter, strict inequalities on both tests, a missing model atom costs score.  It is not
 *     OpenStructure's code, it aligns no sequences, and no test can pin it against OpenStructure itself.
 *
 * All arrays are host memory.
 *   ref_xyz, mob_xyz   double[total][3]: the reference (native) and the model coordinates of all pairs, pair after pair; atom i of
 *                      one list is the same atom as atom i of the other (any value, NaN and infinities included);
 *   residue            int32[total]: the residue index of the atom, local to its pair: 0 at the pair's first atom, non-decreasing, in
 *                      steps of 0 or 1 (a residue's atoms are contiguous);
 *   partner            int32[total]: the index, local to the pair, of the atom with which this one may exchange names, -1 when there
 *                      is none: inside the pair, not the atom itself, in the same residue, and partner[partner[i]] = i.  Under
 *                      TH_LDDT_NO_SYMMETRY it is neither read nor checked and may be NULL;
 *   total              number of atoms, 0 <= total <= 2^31 - 1;
 *   offsets            int64[n_pairs + 1]: pair p owns atoms offsets[p] .. offsets[p + 1]; as for th_lddt.  A pair may be empty;
 *   n_pairs            0 <= n_pairs <= 2^31 - 1;
 *   radius             inclusion radius, finite and > 0 (the published default: 15.0);
 *   thresholds         double[4], each finite and > 0 (the published default: 0.5, 1, 2, 4);
 *   flags              0 or TH_LDDT_NO_SYMMETRY;
 *   atom_out           int32[total][5]: n_i, c_i[0..3]; five zeros at an atom that is not reference-valid;
 *   swapped_out        uint8[total]: 1 where the model coordinates used for this atom were its partner's;
 *   pair_out           int64[n_pairs][8]: n_ref (reference-valid atoms), n_missing, N, C[0..3], n_swapped_residues;
 *   kernel_ms          NULL, or double[2]: the device time in milliseconds of the symmetry resolution and of the counting kernels.
 * The rule, for one pair, all arithmetic float64 and no fused multiply-add:
 *   - REFERENCE-VALID: an atom whose three reference coordinates are finite.  An atom that is not is never an i and never a j, and
 *     its row is zeros;
 *   - MISSING: a reference-valid atom whose model coordinates are not all finite (the kernel makes all three NaN).  It stays in every
 *     count of included pairs and is preserved at no threshold: a missing atom costs score, which is the published behaviour.  This
 *     differs on purpose from th_lddt, which drops such a position;
 *   - DISTANCE  d(a, b) = sqrt((dx*dx + dy*dy) + dz*dz), as for th_lddt;
 *   - an ordered pair (i, j) is INCLUDED when both atoms are reference-valid, residue[i] != residue[j] and d_ref(i, j) < radius.
 *     Strict.  (The kernel compares the squared distance with th_packing_threshold(radius), which decides the same for every double,
 *     and takes square roots of included pairs only.)  There is no self pair to subtract: it lies within one residue;
 *   - an included pair is PRESERVED at threshold t when |d_ref(i, j) - d_mob(i, j)| < t.  Strict;
 *   - SYMMETRY RESOLUTION, unless TH_LDDT_NO_SYMMETRY: for every residue R that has atoms with partner >= 0, keep_R and swap_R are
 *     sums over the atoms a of R that have a partner, over the atoms b with partner[b] < 0 and residue[b] != R, of the (a, b)
 *     included by the reference distance, and over the four thresholds, of the preserved tests of d(mob[a], mob[b]) for keep and of
 *     d(mob[partner[a]], mob[b]) for swap.  R is swapped iff swap_R > keep_R; a tie keeps the names.  A swap exchanges the model
 *     coordinates of all partnered atoms of R together, and all counts are taken on the model after the swaps.  The decisions look
 *     only at atoms without a partner, so they depend neither on one another nor on their order;
 *   - per atom: n_i is the number of included j, c_i[k] the number of those preserved at thresholds[k];
 *   - per pair: n_ref, n_missing, N = sum n_i, C[k] = sum c_i[k] over ORDERED pairs, and the number of swapped residues, 64-bit;
 *   - the caller forms the fractions as for th_lddt: lddt = sum_k C[k] / (4 N), pair-weighted, NaN when N = 0.
 * Out of scope: stereochemistry checks, sequence-separation filters, ligands, sequence alignment, hydrogens, NMR ensembles.
 * All outputs are integers decided by float64 comparisons: a pair's outputs depend on its own arrays alone — not on its place in the
 * batch or on its neighbours — and two calls give the same bytes.  No atomics.  No length limit beyond the 2^31 - 1 atoms of a call.
 * Device memory: 77 bytes per atom + 12 per partnered atom + 8 per 256 atoms of every pair + 88 per pair.  TH_EINVAL, before anything
 * is launched or written: everything th_lddt refuses; a NULL residue, partner (without TH_LDDT_NO_SYMMETRY), atom_out or swapped_out
 * when total > 0; a residue array that breaks the rule above; a partner that is out of its pair, is the atom itself, lies in another
 * residue or fails partner[partner[i]] == i; unknown flag bits.  n_pairs = 0 (with total = 0) is success without a launch. */
#define TH_LDDT_NO_SYMMETRY 1u   /* partner is ignored: the model is scored as named */
int th_lddt_atoms(int device, const double* ref_xyz, const double* mob_xyz, const int32_t* residue, const int32_t* partner,
                  int64_t total, const int64_t* offsets, int64_t n_pairs, double radius, const double* thresholds, unsigned flags,
                  int32_t* atom_out, uint8_t* swapped_out, int64_t* pair_out, double* kernel_ms);

/* ---- *** PARITY UNPINNED AGAINST THE TM-score PROGRAM *** TM-score of models against their native: analyse_models.py --tmscore —
 * the template-modelling score (Zhang & Skolnick 2004), the "scTM against the native" of a design pipeline's self-consistency
 * check.  It is the MAXIMUM over superpositions of sum_i 1 / (1 + (d_i / d0)^2) / L, and the superposition that attains it is in
 * general not the least-squares fit of th_superpose: it has to be searched for.  Here for a BATCH of position-paired coordinate
 * lists, every seed of every pair one wavefront.
 *
 *     *** PARITY UNPINNED AGAINST THE TM-score PROGRAM ***  Zhang & Skolnick's TMscore is not available where this project is built.
 *     The rule below is this project's reading of the PUBLISHED definition and of the published search (fits over windows of the
 *     chain, refined by re-fitting over the positions that came close); it is not their code, it aligns no sequences, and no test can
 *     pin it against their program.
 *
 * All arrays are host memory.  ref_xyz, mob_xyz, total, offsets and n_pairs are exactly those of th_superpose, except that a pair
 * has at most TH_TM_MAX_POSITIONS positions;
 *   norm_len           NULL, or int32[n_pairs]: the normalisation length L of every pair, >= the pair's number of positions (the
 *                      length of the native, when the model lacks residues).  NULL: L is the pair's number of positions;
 *   rounds             refinement rounds per seed at most, >= 0 (the Python layer's default: 20);
 *   tm_out             double[n_pairs][2]: tm, d0;
 *   count_out          int64[n_pairs][4]: n_valid, L, n_seeds, n_fits;
 *   dist_out           double[total] or NULL: d_i under the best superposition, NaN at an invalid position;
 *   transform_out      double[n_pairs][12] or NULL: rows of [R | t] of the best superposition, as th_superpose (the identity when
 *                      no position is valid);
 *   kernel_ms          NULL, or receives the device time of the two kernels (events around them), in milliseconds.
 * The rule, for one pair of n positions ref[i], mob[i], all arithmetic float64 and no fused multiply-add:
 *   - a position is VALID when all six of its coordinates are finite.  m is the number of valid positions; they are kept in index
 *     order, and "position" below means a valid one;
 *   - L = norm_len[p] if given, else n.  d0 = th_tm_d0(L) = max(0.5, 1.24 cbrt(L - 15) - 1.8) for L > 15, else 0.5, computed on the
 *     host.  d_search = min(max(d0, 4.5), 8.0);
 *   - the SCORE of a superposition is (sum over the positions in index order of 1 / (1 + (d_i / d0)^2)) / L, with d_i formed as in
 *     th_superpose: moved = R (mob - cm) + cr, then the square root of the three squares.  (The kernel sums each lane's positions
 *     l, l + 64, ... in index order and then the 64 lanes in a fixed tree.)
 *   - SEEDS: the window lengths are W = m, then W <- W div 2 for as long as the halved value is >= 4; for every W in that order,
 *     every start s = 0 .. m - W is a seed, its set the positions s .. s + W - 1.  n_seeds is their number (239 for m = 76, 1 for
 *     m <= 7);
 *   - per seed, rounds r = 0 .. rounds: FIT over the set by the rule of th_superpose (centroids, two-pass cross-covariance, Horn's
 *     matrix, cyclic Jacobi, the proper rotation); the d_i of all positions and the SCORE; a SCORE strictly greater than the best
 *     so far replaces it.  After round `rounds` the seed ends.  Otherwise cut = d_search - 1 in round 0 and d_search + 1 afterwards,
 *     and the new set is the positions with d_i < cut (strict); while it holds fewer than min(3, m) positions, cut += 0.5 and the
 *     selection is made again (at most TH_TM_MAX_WIDENINGS times — no structure gets there; the seed ends if that is not enough).
 *     If the new set equals the current one the seed ends, otherwise it is the set of the next round.  n_fits counts every fit of
 *     every seed;
 *   - the pair's tm is the best SCORE over its seeds; of equal scores the first seed and round wins.  transform_out and dist_out
 *     are that superposition;
 *   - m = 0 (and a pair none of whose scores is a number): tm is NaN, dist_out NaN and the transform the identity; with m = 0,
 *     n_seeds = n_fits = 0.
 * MIRROR IMAGES: the rotation is proper, so a mirror image scores low here — 0.308 for the mirror case of the superposition
 * fixture, which lDDT (above) scores 1.0 and th_superpose reports as 10.7 Angstrom.  A re-oriented domain costs TM-score only its
 * own positions: the hinge case of that fixture scores 0.904 here, 0.661 under the one global fit of th_superpose, and 0.906 by lDDT.
 * k_tm_seeds runs one wavefront per (pair, seed) with the seed's set as one 64-bit mask per lane in registers (hence 64 x 64 = 4096
 * positions at most) and leaves 12 bytes per seed; k_tm_best, one wavefront per pair, takes the first maximum and runs that one
 * seed again to write the pair's outputs.  No atomics.  A pair's outputs depend on its own coordinates and L alone — not on its
 * place in the batch or on its neighbours — and two calls give the same bytes.  Device memory: 48 bytes per valid position + 4 (12
 * with dist_out) per position + 12 per seed + 104 (200 with transform_out) per pair.  TH_EINVAL, before anything is launched or
 * written: the cases of th_superpose (a negative or too large size, a NULL that is required — offsets, tm_out, count_out; with
 * total > 0 also both lists —, offsets that decrease, do not start at 0 or do not end at total), rounds < 0, a norm_len[p] below the
 * pair's number of positions, a pair of more than TH_TM_MAX_POSITIONS positions, more than 2^31 - 1 seeds in one call.  n_pairs = 0
 * (with total = 0) is success without a launch. */
#define TH_TM_MAX_POSITIONS 4096
#define TH_TM_MAX_WIDENINGS 4096
int th_tmscore(int device, const double* ref_xyz, const double* mob_xyz, int64_t total, const int64_t* offsets, int64_t n_pairs,
               const int32_t* norm_len, int rounds, double* tm_out, int64_t* count_out, double* dist_out, double* transform_out,
               double* kernel_ms);
/* max(0.5, 1.24 cbrt(L - 15) - 1.8) for L > 15, else 0.5: the scale d0 of the TM-score for normalisation length L.  Host code. */
double th_tm_d0(int64_t L);

/* ---- *** PARITY UNPINNED AGAINST PYMOL *** structural alignment of models of any length: analyse_models.py --cealign — the
 * reference's calculate_RMSD_and_gdt / _calculate_RMSD of scripts/analyse_all_properties.py and
 * scripts/analyse_cherrypicked_samples_af2.py, which call PyMOL's cmd.cealign on the CA atoms: a sequence-independent alignment by
 * combinatorial extension (CE, Shindyalov & Bourne 1998).  Here for a BATCH of (reference, model) pairs whose two lengths are
 * independent.  The alignment is a pairing: th_superpose, th_lddt and th_tmscore score it unchanged.
 *
 *     *** PARITY UNPINNED AGAINST PYMOL ***  PyMOL is not available where this project is built.  The rule below is this project's
 *     reading of the PUBLISHED algorithm with cealign's documented defaults (window 8, d0 3.0, d1 4.0, gap_max 30, the best 20 paths
 *     re-scored by RMSD); it is not PyMOL's code and no test can pin it against PyMOL.
 *
 * All arrays are host memory.
 *   ref_xyz            double[ref_total][3]: the reference (native) coordinates of all pairs, pair after pair (any value);
 *   ref_offsets        int64[n_pairs + 1]: pair p owns positions ref_offsets[p] .. ref_offsets[p + 1]; from 0 to ref_total, never
 *                      decreasing; a structure may be empty and has at most TH_CE_MAX_POSITIONS positions;
 *   mob_xyz, mob_total, mob_offsets   the same for the models;
 *   n_pairs            0 <= n_pairs <= 2^31 - 1, as are both totals;
 *   d0, d1             the similarity thresholds of a fragment pair and of a path, finite and > 0 (cealign's: 3.0 and 4.0);
 *   gap_max            0 .. 31 (cealign's: 30): the 2 gap_max + 1 candidates of a step are the lanes of one wavefront;
 *   align_out          int32[ref_total]: the index, local to the pair, of the model position aligned to this reference position,
 *                      -1 if none;
 *   score_out          double[n_pairs][2]: the RMSD over the aligned positions, the winning path's score;
 *   count_out          int64[n_pairs][6]: mA, mB, n_starts, n_afps, n_aligned, n_candidates;
 *   transform_out      double[n_pairs][12] or NULL: rows of [R | t] of the winning fit, as th_superpose (the identity without a start);
 *   kernel_ms          NULL, or receives the device time of the four kernels (events around them), in milliseconds.
 * The rule, for one pair — A the reference with nA positions, B the model with nB —, all arithmetic float64 and
 * no fused multiply-add: every product, sum and quotient is rounded on its own, square roots are correctly rounded.  W = TH_CE_WINDOW = 8.
 *   1. VALID: a position is valid when its three coordinates are finite.  Each list is compacted to its valid positions in index
 *      order, mA and mB of them; "position" below means a compacted one; outputs are in the caller's original indices.
 *   2. DISTANCE inside one structure: d(i, j) = sqrt((dx*dx + dy*dy) + dz*dz).
 *   3. WINDOW STARTS: a = 0 .. mA - W and b = 0 .. mB - W; none when mA < W or mB < W.
 *   4. SIMILARITY: over the 21 pairs (p, q), 0 <= p, q >= p + 2, q <= 7, in lexicographic order,
 *      S(a, b) = (sum |dA(a + p, a + q) - dB(b + p, b + q)|) / 21, the terms added left to right.
 *   5. STARTS: every (a0, b0) with S(a0, b0) < d0, strict; n_starts counts them; a start's index is a0 (mB - W + 1) + b0.
 *   6. DISTANCE OF TWO FRAGMENT PAIRS (CE's independent set, W terms):
 *      D((ai, bi), (aj, bj)) = (|dA(ai, aj) - dB(bi, bj)| + |dA(ai + 7, aj + 7) - dB(bi + 7, bj + 7)|
 *                               + sum over k = 1 .. 6 of |dA(ai + k, aj + 7 - k) - dB(bi + k, bj + 7 - k)|) / 8, added in that order.
 *   7. PATH from a start: path = [(a0, b0)], sumS = S(a0, b0), sumD = 0.  Repeat, with n AFPs (aligned fragment pairs) so far and
 *      the last at (a, b): the candidates are g = 0 .. 2 gap_max — g = 0: (a + W, b + W); odd g: (a + W + (g + 1) / 2, b + W); even
 *      g > 0: (a + W, b + W + g / 2).  A candidate counts only when it is a window start of both sides and its S < d0.  Its cost is
 *      c = s / n with s = sum over k ascending of D(path[k], candidate); it is eligible when c < d1.  The eligible candidate of
 *      smallest c is taken, of equal costs the smallest g; without one the path ends.  score = ((sumS + S(cand)) + (sumD + s)) /
 *      ((n + 1) + (n + 1) n / 2); if that is not < d1 the path ends WITHOUT the candidate; otherwise the candidate is appended,
 *      sumS += S(cand), sumD += s.  A path's score is (sumS + sumD) / (n + n (n - 1) / 2).
 *   8. CANDIDATES: all paths ordered by length descending, then score ascending, then start index ascending; the first
 *      n_candidates = min(TH_CE_KEEP, n_starts) are the candidates.
 *   9. WINNER: each candidate is fitted by the rule of th_superpose (centroids, two-pass cross-covariance, Horn's matrix, cyclic
 *      Jacobi, the proper rotation) over its 8 n aligned position pairs; every sum of the fit runs over the pairs in path order, one
 *      after the other (no tree: among near-identical candidates the order of addition decides); its RMSD is sqrt(sum d_i^2 / (8 n)).  The candidate of smallest RMSD
 *      wins, of equal RMSDs the first in candidate order.  n_afps = n, n_aligned = 8 n.
 *  10. NO START: n_afps = n_aligned = n_candidates = 0, the RMSD and the score are NaN, the transform is the identity and nothing
 *      is aligned.  That is a result, not an error.
 * MIRROR IMAGES: CE compares distances and does not see a mirror image; the proper rotation then refuses to fit it (64 aligned
 * positions at 9.55 Angstrom for the mirror case of the superposition fixture).  An ideal helix against an ideal strand has no start.
 * k_ce_windows writes the 21 distances of every window start, k_ce_similarity S in 16 x 16 tiles with the rows staged in LDS,
 * k_ce_paths runs one wavefront per (a0, b0) — lane g evaluates candidate g, the path lives in registers, at most 256 AFPs —
 * and leaves 12 bytes per (a0, b0); k_ce_best, one wavefront per pair, selects the candidates by rule 8, traces each again, fits it
 * and writes the winner.  No atomics.  A pair's outputs depend on its own coordinates alone — not on its place in the batch or on
 * its neighbours — and two calls give the same bytes.  Device memory per pair: (mA - 7)(mB - 7) * 8 bytes for S — the dominant
 * term, 33 MB at 2048 x 2048 — and 12 more per (a0, b0) for the paths' records, 168 bytes per window start of either side, 28 per
 * valid position, 4 per reference position and 160 (256 with transform_out) per pair.  TH_EINVAL, before anything is launched or
 * written: a negative or too large size, a NULL that is required (both offsets, score_out, count_out; with ref_total > 0 also
 * ref_xyz and align_out, with mob_total > 0 also mob_xyz), offsets of either list that decrease, do not start at 0 or do not end at
 * the list's total, d0 or d1 not finite or <= 0, gap_max < 0 or > 31, a structure of more than TH_CE_MAX_POSITIONS positions, more
 * than 2^33 - 4 window pairs in one call.  n_pairs = 0 (with both totals 0) is success without a launch. */
#define TH_CE_MAX_POSITIONS 2048      /* per structure */
#define TH_CE_WINDOW 8
#define TH_CE_KEEP 20
int th_cealign(int device, const double* ref_xyz, int64_t ref_total, const int64_t* ref_offsets, const double* mob_xyz, int64_t mob_total,
               const int64_t* mob_offsets, int64_t n_pairs, double d0, double d1, int gap_max, int32_t* align_out, double* score_out,
               int64_t* count_out, double* transform_out, double* kernel_ms);

/* ---- *** PARITY UNPINNED AGAINST PYMOL *** sequence alignment of models to their native: analyse_models.py --seqalign and
 * --pair_by_seqalign — the pairing that survives renumbering, a missing loop and a purification tag together, and that exists for a
 * misfolded model too.  The reference's scripts/analyse_af2.py calls PyMOL's cmd.align, a sequence alignment followed by a fit;
 * th_superpose is the fit, this is the alignment.  cmd.align's own recurrences, end-gap treatment and tie handling are not available
 * to pin against: the rule below is this project's own, a global alignment with affine gap costs (Gotoh's three tables) whose end
 * gaps are free or charged, all in integers.  Here for a BATCH of (reference, model) pairs in one call, one wavefront per pair.
 *
 * All arrays are host memory.
 *   ref_codes          uint8[ref_total]: the references, pair after pair.  A residue is one byte: 0..19 are the letters
 *                      ACDEFGHIKLMNPQRSTVWY, 20 is anything else (the coding of th_seqset); a byte above 20 is refused, naming its index;
 *   ref_offsets        int64[n_pairs + 1]: pair k owns residues ref_offsets[k] .. ref_offsets[k + 1]; from 0 to ref_total, never
 *                      decreasing; a sequence may be empty and has at most TH_SEQALIGN_MAX_LENGTH residues;
 *   mob_codes, mob_total, mob_offsets   the same for the models;
 *   n_pairs            0 <= n_pairs <= 2^31 - 1, as are both totals;
 *   matrix             int32[21][21]: the substitution table S, row = the reference's code, every entry within -127 .. 127 (the
 *                      Python default is 2 x BLOSUM62 with -2 wherever either code is 20: cmd.align's documented gap = -10 and
 *                      extend = -0.5 then are the integers gap_open = 20 and gap_extend = 1);
 *   gap_open, gap_extend   0 <= gap_extend <= gap_open <= 32767: a run of k unpaired residues costs gap_open + (k - 1) gap_extend;
 *   free_ends          1: unpaired residues before the first and after the last cell of the path cost nothing; 0: global;
 *   align_out          int32[ref_total]: the index, local to the pair, of the model residue aligned to this reference residue, -1 if
 *                      none (the convention of th_cealign);
 *   count_out          int64[n_pairs][8]: n_ref, n_model, score, n_aligned, n_identical (aligned and the two bytes equal),
 *                      n_positive (aligned with S > 0), n_gaps (runs of unpaired residues of either side strictly between the first
 *                      and the last aligned pair; a run of each side between the same two pairs counts twice), n_gap_residues;
 *   kernel_ms          NULL, or double[2]: the device time (events) of the fill and of the trace, in milliseconds.
 * The rule, for one pair — reference a[1..n], model b[1..m] —, three values per cell, "minus infinity" = -2^30:
 *   1. E[i][j] = max(H[i][j-1] - gap_open, E[i][j-1] - gap_extend): model residue j unpaired.  The cell's E is marked EXTENDED
 *      only when the second term is strictly greater.
 *   2. F[i][j] = max(H[i-1][j] - gap_open, F[i-1][j] - gap_extend): reference residue i unpaired; EXTENDED likewise.
 *   3. H[i][j] starts as H[i-1][j-1] + S[a_i][b_j]; F[i][j] replaces it only if strictly greater; then E[i][j] replaces it only if
 *      strictly greater.  The ORIGIN (diagonal / F / E) is recorded.
 *   4. BORDERS.  free_ends = 1: H[i][0] = H[0][j] = 0, and E, F on the border are minus infinity.  free_ends = 0: H[0][0] = 0,
 *      H[i][0] = F[i][0] = -(gap_open + (i - 1) gap_extend), H[0][j] = E[0][j] = -(gap_open + (j - 1) gap_extend); E[i][0] for i > 0
 *      and F[0][j] for j > 0 are minus infinity.
 *   5. END CELL.  Global: (n, m).  Free ends: the maximum of H over the last row and the last column, scanned (n, m) first, then
 *      (n, j) for j = m - 1 .. 0, then (i, m) for i = n - 1 .. 0; a later cell wins only if strictly greater.  score = H there.
 *   6. TRACE from the end cell in state H.  In state H read the origin: diagonal pairs a_i with b_j and moves to (i - 1, j - 1);
 *      origin F or E enters that state.  In state F read the EXTENDED bit of F at (i, j), move to (i - 1, j), and stay in F if it
 *      was set, else return to H; E is the same along j.  Stop when i = 0 or j = 0: whatever is left on a border is unpaired.
 * The score is the sum of S over the aligned pairs minus the cost of every run on the path.  With free ends the path lies between
 * the border cell where the trace stops and the end cell; a run of ONE side may precede its first pair or follow its last (two
 * overhangs cannot both be skipped for nothing) and is charged, but is not among n_gaps.  An empty sequence aligns nothing and scores
 * 0, or minus the border cost in global mode.
 * k_seqalign_fill: lane l of the pair's wavefront owns a strip of 8 model columns and works on reference row t - l at step t; H and
 * F of the strip stay in registers, the strip's right edge goes to lane l + 1 by a cross-lane move, the 8 scores of a step are one
 * 8-byte LDS read, columns beyond 512 are further panels whose edge column is carried in memory, and the four trace bits of a cell
 * are packed eight cells to a dword.  k_seqalign_trace: one thread per pair walks the bits back.  All integers, no atomics, no float
 * arithmetic: a pair's bytes are the same wherever it sits in a batch.  Device memory per pair: the trace bits — 4 (n + s - 1) s
 * bytes for the last panel of s = ceil(columns / 8) strips and 256 (n + 63) for every whole panel before it, 3.4 KB at 76 x 76 and
 * 8.5 MB at 4096 x 4096 —, 17 bytes per reference residue, 5 per model residue, 120 per pair.  TH_EINVAL, before any device call:
 * a negative or too large size, a NULL that is required (both offsets, matrix, count_out; with ref_total > 0 ref_codes and
 * align_out, with mob_total > 0 mob_codes), offsets of either list that decrease, do not start at 0 or do not end at the list's
 * total, a code above 20, gap_open < gap_extend, gap_extend < 0, gap_open > 32767, free_ends neither 0 nor 1, a table entry outside
 * -127 .. 127, a sequence of more than TH_SEQALIGN_MAX_LENGTH residues (the score then stays below 2^28 and the trace bits below
 * 8.5 MB).  n_pairs = 0 (with both totals 0) is success without a launch. */
#define TH_SEQALIGN_MAX_LENGTH 4096   /* per sequence */
int th_seqalign(int device, const uint8_t* ref_codes, int64_t ref_total, const int64_t* ref_offsets, const uint8_t* mob_codes,
                int64_t mob_total, const int64_t* mob_offsets, int64_t n_pairs, const int32_t* matrix, int gap_open, int gap_extend,
                int free_ends, int32_t* align_out, int64_t* count_out, double* kernel_ms);

/* ---- *** PARITY UNPINNED AGAINST DSSP *** secondary structure of protein backbones: analyse_properties.py --secondary_structure and
 * analyse_models.py --secondary_structure — where the helices and strands are, by the DSSP rule (Kabsch & Sander 1983): backbone
 * hydrogen bonds by an electrostatic energy, then turns, helices, bridges, ladders and bends as patterns of those bonds.  What the
 * reference leaves to PyMOL pictures.  Here for a BATCH of structures in one call: an all-pairs float64 pass over the residues of
 * each structure, then integer pattern matching.
 *
 *     *** PARITY UNPINNED AGAINST DSSP ***  (mkdssp, PyMOL's dss, STRIDE.)  None of them is available where this project is built.
 *     The rule below is this project's reading of the PUBLISHED definition and not their code.  Those programs' tie rules, bulges,
 *     G / I precedence and bond caps differ in detail: assignments can differ at helix ends and sheet edges, and no test can pin
 *     this rule against mkdssp.
 *
 * All arrays are host memory.
 *   backbone           double[total][4][3]: N, CA, C, O of every residue, structure after structure, in the caller's order (any value;
 *                      NaN for an atom the residue lacks);
 *   chain              int32[total]: a chain id; a change of id is a chain break;
 *   no_h               uint8[total]: non-zero for a residue whose N carries no hydrogen (proline);
 *   total              number of residues, 0 <= total <= 2^31 - 1;
 *   offsets            int64[n_structures + 1]: structure s owns residues offsets[s] .. offsets[s + 1]; offsets[0] = 0, non-decreasing,
 *                      offsets[n_structures] = total.  A structure may be empty.  There is no length limit;
 *   n_structures       0 <= n_structures <= 2^31 - 1;
 *   class_out          uint8[total]: 0 '-', 1 H, 2 B, 3 E, 4 G, 5 I, 6 T, 7 S;
 *   residue_out        int32[total][6]: the two lowest bridge partners as structure-local indices (or -1); flags (bits 0-2: a 3-, 4-,
 *                      5-turn starts here, 3: bend, 4: has a parallel bridge, 5: has an antiparallel bridge, 6: conn(i), 7: valid);
 *                      bonds accepted (as C=O); bonds donated (as N-H); the number of bridge partners;
 *   structure_out      int64[n_structures][10]: n_valid, n_hbonds, then the number of residues of each of the eight classes;
 *   hbond_bits_out     NULL, or uint64[sum over s of L_s * ceil(L_s / 64)]: the hydrogen bonds.  Structure s has L_s rows of
 *                      ceil(L_s / 64) words, row = acceptor, bit (d & 63) of word (d >> 6) = donor d, both structure-local, and starts
 *                      at word sum over t < s of L_t * ceil(L_t / 64);
 *   kernel_ms          NULL, or double[3]: the device time (events) of the hydrogen-bond pass (with the per-residue preparation), of
 *                      the assignment and of the totals, in milliseconds.
 * The rule, for one structure of residues 0 .. L-1, all arithmetic float64 and no fused multiply-add:
 *   - VALID(i): all 12 coordinates are finite.  An invalid residue makes no bond, is a break on both sides and gets class '-';
 *   - CONN(i), the link i -> i+1: both residues are valid, have the same chain id, and the squared C(i)-N(i+1) distance is <= 6.25;
 *   - H(i) = N(i) + v / |v| with v = C(i-1) - O(i-1), each component divided by |v| = sqrt((vx*vx + vy*vy) + vz*vz).  It exists only
 *     where conn(i-1) holds, no_h is false and its three components are finite (a C on its own O has none).  A residue without H
 *     donates nothing;
 *   - ENERGY of acceptor a (C=O) and donor d (N-H), taken only when a is valid, d has H, d != a, d != a + 1 and the squared CA-CA
 *     distance is < 81.0.  Every distance is sqrt((dx*dx + dy*dy) + dz*dz).  q = ((1/rON + 1/rCH) - 1/rOH) - 1/rCN;
 *     e = (int)floor((27.888 * q) * 1000 + 0.5), in milli-kcal/mol; if any of the four distances is < 0.5 then e = -9900; e is never
 *     below -9900.  HB(a, d) <=> e < -500.  ALL bonds count: there is no "two best per residue" cap, which is mkdssp's book-keeping
 *     and not the definition;
 *   - TURN_n(i), n = 3, 4, 5: hb(i, i+n) and conn(i) .. conn(i+n-1);
 *   - HELICES: turn_4(i-1) and turn_4(i) => H at i .. i+3; turn_3(i-1) and turn_3(i) => G at i .. i+2; turn_5(i-1) and turn_5(i) => I
 *     at i .. i+4; turn_n(i) => T at i+1 .. i+n-1;
 *   - BRIDGES, for |i - j| >= 3 with conn(i-1), conn(i), conn(j-1), conn(j); the chains may differ.
 *     parallel <=> [hb(i-1, j) and hb(j, i+1)] or [hb(j-1, i) and hb(i, j+1)];
 *     antiparallel <=> [hb(i, j) and hb(j, i)] or [hb(i-1, j+1) and hb(j-1, i+1)];
 *   - E or B: residue i is E when it has a parallel bridge to some j and (i+1, j+1) or (i-1, j-1) is also a parallel bridge, or an
 *     antiparallel bridge to some j and (i+1, j-1) or (i-1, j+1) is also an antiparallel bridge.  A bridged residue that is not E
 *     is B.  Beta-bulges are NOT bridged over (out of scope), and sheets are not labelled;
 *   - S: conn(i-2) .. conn(i+1) hold and dot(a, b) / (|a| * |b|) < 0.3420201433256688 with a = CA(i) - CA(i-2), b = CA(i+2) - CA(i):
 *     a bend of more than 70 degrees.  No trigonometry anywhere;
 *   - PRIORITY per residue: H > E > B > G > I > T > S > '-'.  Three-state reduction (the caller's): H, G, I -> helix; E, B -> strand;
 *     the rest -> coil.
 * All outputs are integers decided by float64 comparisons: a structure's outputs depend on its own residues alone — not on its place
 * in the batch or on its neighbours — and two calls give the same bytes.  No atomics.  Device memory: 151 bytes per residue, 8 per
 * 256 residues of every structure, 96 per structure and the bitmap, L * ceil(L / 64) * 8 bytes per structure; a device that cannot
 * hold them is TH_ENOMEM.  TH_EINVAL, before anything is launched or written: a negative or too large size, a NULL that is required
 * (offsets, structure_out; with total > 0 also backbone, chain, no_h, class_out and residue_out), offsets that decrease, do not start
 * at 0 or do not end at total.  n_structures = 0 (with total = 0) is success without a launch. */
int th_secondary_structure(int device, const double* backbone, const int32_t* chain, const uint8_t* no_h, int64_t total,
                           const int64_t* offsets, int64_t n_structures, uint8_t* class_out, int32_t* residue_out, int64_t* structure_out,
                           uint64_t* hbond_bits_out, double* kernel_ms);

/* ---- *** PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON *** solvent-accessible surface area of structures:
 * analyse_properties.py --sasa and analyse_models.py --sasa — which atoms and residues are buried and which face the solvent, by the
 * numerical method of Shrake & Rupley (1973): every atom carries a sphere of its van der Waals radius plus a probe radius with test
 * points on it, and a point is exposed unless it lies inside the sphere of another atom.  The only burial measure the reference has
 * is its contact number (th_packing_density).  Here for a BATCH of structures in one call.
 *
 *     *** PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON ***  None of them is available where this project is built
 *     (verified absent: the Python modules Bio, freesasa and mdtraj).  The rule below is this project's own.  Those programs use
 *     their own radii, point sets (or Lee-Richards slices) and tie rules: areas differ from theirs by the usual few per cent between
 *     SASA programs, and no test can pin this rule against them.
 *
 * All arrays are host memory.
 *   xyz                double[total][3]: the atoms, structure after structure, in the caller's order (any value);
 *   radius             double[total]: the van der Waals radius of each atom (any value);
 *   total              number of atoms, 0 <= total <= 2^31 - 257;
 *   offsets            int64[n_structures + 1]: structure s owns atoms offsets[s] .. offsets[s + 1]; offsets[0] = 0, non-decreasing,
 *                      offsets[n_structures] = total.  A structure may be empty.  There is no length limit;
 *   n_structures       0 <= n_structures <= 2^31 - 1;
 *   probe              the probe radius (1.4 for water; 0 gives the van der Waals surface; any value);
 *   points             double[n_points][3]: the directions u_k, the caller's, normally of unit length (th_sasa_sphere); all finite;
 *   n_points           1 <= n_points <= 1024;
 *   exposed_out        int32[total]: the number of exposed points of every atom, -1 for an invalid atom;
 *   mask_out           NULL, or uint64[total][ceil(n_points / 64)]: bit (k & 63) of word (k >> 6) is set where point k is exposed;
 *                      padding bits are 0, all words of an invalid atom are 0;
 *   structure_out      int64[n_structures][3]: valid atoms, valid atoms with no exposed point, the sum of exposed_out over valid atoms;
 *   kernel_ms_out      NULL, or double[2]: the device time (events) of the occlusion pass and of the totals, in milliseconds.
 * The rule, for one structure of atoms 0 .. n-1, all arithmetic float64, every product, sum and difference rounded on its own in the
 * written order (no fused multiply-add):
 *   - EXPANDED RADIUS: R_i = radius_i + probe;
 *   - VALID(i): the three coordinates and R_i are finite and R_i > 0.  An invalid atom occludes nothing, its count is -1 and its mask
 *     words are 0;
 *   - NEAR(i, j): j != i, the same structure, both valid, and s < t*t, strict, with dx = x_j - x_i, dy = y_j - y_i, dz = z_j - z_i,
 *     s = (dx*dx + dy*dy) + dz*dz and t = R_i + R_j.  This pre-filter is PART OF THE RULE, not an optimisation assumed harmless: an
 *     atom that is not near occludes nothing, whatever its sphere does in rounded arithmetic;
 *   - SPHERE POINT k of atom i: p_k = (x_i + R_i*u_kx, y_i + R_i*u_ky, z_i + R_i*u_kz);
 *   - OCCLUSION: point k of atom i is buried <=> some j with near(i, j) has (ex*ex + ey*ey) + ez*ez < R_j*R_j, strict, with
 *     e = p_k - c_j, the centre of j.  A point exactly on a neighbour's sphere is exposed;
 *   - COUNT: exposed_out[i] = the number of points that are not buried.  MASK: which ones.
 *   Consequences: coincident atoms of equal radius bury each other's points only as far as the rounding of |u_k| decides (of 96
 *   golden-spiral points 76 survive for two atoms of R = 3.1 at the origin, 80 for R = 3 at (1, 2, 3), 51 inside a protein's
 *   coordinates): deterministic and physically meaningless.  A sphere wholly inside another gets 0.  Distances that
 *   overflow to infinity are not near.  The neighbours are all pairs of the structure: no cell grid and no neighbour list, so no
 *   capacity either — 300 atoms on one spot are 300 neighbours.
 * AREAS are the caller's, in float64: area_i = exposed_i * (4 * pi * R_i * R_i / n_points), multiplied left to right (0 for an
 * invalid atom), and a residue's area is the sequential sum over its atoms in file order (timed_hip/sasa.py).
 * All device outputs are integers and bit sets decided by float64 comparisons, and an AND over neighbours whose order cannot change a
 * bit: a structure's outputs depend on its own atoms alone — not on its place in the batch or on its neighbours — and two calls give
 * the same bytes.  No atomics.  Device memory: 32 bytes per atom in, 4 + 8 * ceil(n_points / 64) bytes per atom out (4 without
 * mask_out), 2 per atom of work items, 32 per structure and 24 per point; a device that cannot hold them is TH_ENOMEM.  TH_EINVAL,
 * before anything is launched or written: a negative or too large size, n_points outside 1 .. 1024, a point coordinate that is not
 * finite, a NULL that is required (points; with n_structures > 0 offsets and structure_out; with total > 0 also xyz, radius and
 * exposed_out), offsets that decrease, do not start at 0 or do not end at total.  total = 0 is success without a launch. */
int th_sasa(int device, const double* xyz, const double* radius, int64_t total, const int64_t* offsets, int64_t n_structures,
            double probe, const double* points, int32_t n_points, int32_t* exposed_out, uint64_t* mask_out, int64_t* structure_out,
            double* kernel_ms_out);
/* The golden spiral: n_points directions spread evenly over the unit sphere, computed with the host's libm (host code, no GPU).  For
 * k = 0 .. n_points - 1: z = 1 - (2k + 1) / n_points, rho = sqrt(1 - z*z), phi = k * (pi * (3 - sqrt(5))), u_k = (rho cos phi,
 * rho sin phi, z) into points_out[3k ..].  The points are an INPUT of th_sasa so that the kernel and whoever checks it see the same
 * doubles.  TH_EINVAL: n_points outside 1 .. 1024 or points_out NULL. */
int th_sasa_sphere(int32_t n_points, double* points_out);

/* ---- diversity and native recovery of sampled sequences: analyse_samples.py — what sample.py's draws look like as a set.  The
 * reference reports, in ui.py, accuracy_score(list(seq), list(native)) as "Sequence Identity", the share of positions with
 * lookup_blosum62(a, b) > 0 as "Sequence Similarity" and a sequence logo; how different the draws are from one another, which are the
 * same sequence twice and which few to fold it leaves to the reader.  Here for a BATCH of sets in one call.
 *
 *     The clustering below is the incremental scheme of CD-HIT-like tools in its plainest form.  It is THIS PROJECT'S OWN RULE, NOT
 *     THEIR CODE: no word filter, no length sorting and no alignment — the draws of one structure are position-paired by construction.
 *
 * All arrays are host memory.
 *   codes              uint8[total_codes]: set after set, a set's N sequences of its length L row-major.  A residue is one byte: 0..19
 *                      are the letters ACDEFGHIKLMNPQRSTVWY, 20 is any other letter; a byte above 20 is refused, naming its index;
 *   total_codes        the sum of N_s * L_s over the sets;
 *   seq_offsets        int64[n_sets + 1]: set s owns sequences seq_offsets[s] .. seq_offsets[s + 1]; from 0, non-decreasing, at most
 *                      2^31 - 1 sequences in all.  A set may be empty (N = 0);
 *   lengths            int32[n_sets]: L_s >= 1, and N_s * L_s <= 2^31 - 1;
 *   n_sets             0 <= n_sets <= 2^31 - 1;
 *   native             NULL, or uint8[sum of L_s]: the native sequence of every set, in the same codes;
 *   substitution       int8[20 * 20], row = the native's code: required with a native (timed_hip.analysis.BLOSUM62 — the kernel and
 *                      whoever checks it read the same integers);
 *   min_matches        NULL (no clustering), or int32[n_sets]: 0 <= min_matches[s] <= L_s;
 *   seq_out            int32[sequences][8], below;
 *   profile_out        int32[sum of L_s][21]: how many of the set's sequences hold each code at that position;
 *   matrix_out         NULL, or int32: the N x N block of M of every set, set s at offset sum_{t<s} N_t^2; at most 2^31 - 1 entries;
 *   set_out            int64[n_sets][4], below;
 *   kernel_ms          NULL, or double[3]: the device time (events) of the kernels up to the clustering, of the clustering and of the
 *                      totals, in milliseconds; their sum is the time from the first kernel to the last.
 * The rule, for one set of sequences 0 .. N-1:
 *   - PAIR MATCHES: M(i, j) = the number of positions at which i and j hold the same byte.  Identity is of the letters as written:
 *     code 20 equals code 20;
 *   - seq_out[i]: 0 native_identical = positions equal to the native; 1 native_similar = positions where both codes are below 20 and
 *     substitution[native][seq] > 0; 2 native_score = the sum of substitution[native][seq] over the positions where both codes are
 *     below 20; 3 pair_sum = sum_{j != i} M(i, j); 4 nearest_matches = max_{j != i} M(i, j), -1 when N = 1; 5 nearest_index = the
 *     lowest j != i attaining it, -1 when N = 1; 6 first_equal = the lowest j with M(i, j) = L — the self pair counts, so
 *     first_equal <= i, and i is a distinct sequence iff first_equal == i; 7 cluster.  Without a native columns 0 .. 2 are 0;
 *   - CLUSTERING, greedy, in input order: sequence n joins the lowest-indexed representative r < n with M(n, r) >= min_matches[s];
 *     otherwise it becomes a representative.  cluster = the representative's index, its own for a representative; -1 everywhere
 *     when min_matches is NULL.  The threshold is an integer: an identity is turned into one by the caller (timed_hip/seqset.py:
 *     ceil(p * L / 1000) of the per-mille p, in integer arithmetic);
 *   - set_out[s]: sum_{i<j} M(i, j); the number of distinct sequences; the number of clusters (-1 without); sum_i native_identical.
 * Everything is an integer and no atomics are used: a set's bytes are the same wherever it sits in a batch and whether or not the
 * matrix is asked for.  All pairs cost N^2 * L residue comparisons, four per packed compare.  Device memory: about 2 L + 36 bytes per
 * sequence, 85 per position, 56 per set, 4 N^2 with the matrix; a device that cannot hold them is TH_ENOMEM.  TH_EINVAL, before
 * anything is launched or written: a negative size; total_codes that is not the sum of N_s * L_s; L_s < 1; N_s * L_s, the number of
 * sequences or (with matrix_out) the sum of N_s^2 above 2^31 - 1; a code above 20 in codes or native; min_matches[s] outside
 * 0 .. L_s; a NULL that the sizes need (with n_sets > 0 seq_offsets, lengths, set_out and profile_out; with sequences seq_out; with
 * residues codes); seq_offsets that decrease or do not start at 0; native without substitution.  n_sets = 0 with nothing else is
 * TH_OK. */
int th_seqset(int device, const uint8_t* codes, int64_t total_codes, const int64_t* seq_offsets, const int32_t* lengths,
              int64_t n_sets, const uint8_t* native, const int8_t* substitution, const int32_t* min_matches, int32_t* seq_out,
              int32_t* profile_out, int32_t* matrix_out, int64_t* set_out, double* kernel_ms);
/* The tiles of th_seqset's pair kernel into tiles_out[3]: sequences per row tile, sequences per column tile, positions per staged
 * chunk (host code, no GPU) — so that a test can tell whether its shapes cross them.  TH_EINVAL: tiles_out NULL. */
int th_seqset_tiles(int32_t* tiles_out);
/* The tiles of the Winograd GEMM kernels of the 5^3 layers (csrc/conv_wino.hip: k_wino_gemm, k_wino_gemm_b3_16 / _b3_32 and, with
 * 32-frame row blocks of one 32-column tile, k_wino_gemm_n32) into tiles_out[3]: frames per row block (64; a launch's rows are the
 * frames rounded up to it), output channels per column block (128; four waves of 32 columns, a wave whose columns are all padding
 * stays idle), input channels per staged chunk (32; a layer's Cin is padded up to it) — host code, no GPU, so that the case table of
 * the tests (tests/wino_cases.py) can tell which blocks, chunks and ragged edges its shapes reach, and fails when a tile changes.
 * TH_EINVAL: tiles_out NULL. */
int th_conv_wino_tiles(int32_t* tiles_out);

/* ---- frame ingest: replaces the per-residue h5py reads of load_batch — design_utils/utils.py:514-529.  Host code
 * only.  `file` is the whole HDF5 file in memory (an mmap), `base` its superblock offset.  For n_datasets chunked
 * datasets that share one geometry (shape[rank], chunk[rank], element size, filter pipeline ids in write order:
 * 1 deflate, 2 shuffle, 3 fletcher32) and whose chunk B-trees (version 1) start at btree_addrs[i], inflate every
 * chunk and scatter it into dests[i] (C order, shape[] elements of esz bytes) on nthreads host threads (0 = all
 * usable CPUs — th_host_cpus() —, at most 128).  Unallocated chunks read as zeros.  TH_EUNSUP when the file uses something else (the
 * caller then reads through its generic path). */
int th_h5_read_chunked(const void* file, int64_t file_len, int64_t base, int64_t n_datasets, const int64_t* btree_addrs,
                       void* const* dests, int rank, const int64_t* shape, const int64_t* chunk, int esz, int n_filters,
                       const int* filter_ids, int nthreads);

/* the same with a conversion while the chunks are placed: conv 0 = bytes as stored, 1 = float64 -> float32 (round to
 * nearest even: exactly the cast Keras applies to load_batch's float64 frames; halves the host->device bytes) */
int th_h5_read_chunked_as(const void* file, int64_t file_len, int64_t base, int64_t n_datasets, const int64_t* btree_addrs,
                          void* const* dests, int rank, const int64_t* shape, const int64_t* chunk, int esz, int n_filters,
                          const int* filter_ids, int nthreads, int conv);
/* contiguous (unchunked, unfiltered) datasets: data_addrs[i] = file address of `count` elements of `esz` bytes, -1 = never
 * written (zeros) */
int th_h5_read_contiguous_as(const void* file, int64_t file_len, int64_t base, int64_t n_datasets, const int64_t* data_addrs,
                             void* const* dests, int64_t count, int esz, int conv);
/* The same datasets decoded ON THE DEVICE (f-1: the host's inflate rate — 1.3 k frames/s per core — is what limits predict.py on
 * real gzip .hdf5 datasets, reference design_utils/utils.py:514-529).  Only the chunk B-trees are walked on the host; the
 * COMPRESSED chunk bytes are copied to the GPU as they lie in the file, inflated there one lane per chunk, and placed into d_out —
 * device memory on `device`, [n_datasets][shape...] of float32 when conv = 1 (float64 data: the cast Keras applies) or of the
 * stored element type when conv = 0.  Supports the pipeline aposteriori writes (n_filters = 1, filter id 1 = deflate, every chunk
 * compressed) and shuffle + deflate (filter ids {2, 1}: h5py's compression="gzip", shuffle=True; chunks up to 60 KB); TH_EUNSUP
 * for anything else (use th_h5_read_chunked_as).  Every chunk's Adler-32 is verified as zlib does: a chunk that does not inflate
 * to its declared size or fails the check is TH_EIO.  Never-allocated chunks read as zeros.  Synchronous. */
int th_h5_decode_device(const void* file, int64_t file_len, int64_t base, int64_t n_datasets, const int64_t* btree_addrs, int rank,
                        const int64_t* shape, const int64_t* chunk, int esz, int n_filters, const int* filter_ids, int conv, int device,
                        void* d_out);
/* th_model_free keeps a model's device blocks (weights, arenas, rings) in a per-process cache for the next th_model_load
 * (hipFree synchronises the device: ~13 ms per TIMED handle, paid by every predict.py call that loads and frees a model as
 * reference predict.py:114-121 does); at most min(24 GB, an eighth of the device's memory) are kept per device, the blocks parked
 * longest ago leave first, and every allocator inside the library returns the cache to HIP and retries before it reports
 * TH_ENOMEM.  th_dev_trim returns the cached blocks of `device` (all devices when negative) to HIP; th_dev_cache_info reports
 * what is parked (bytes, the cap, number of blocks). */
int th_dev_trim(int device);
int th_dev_cache_info(int device, uint64_t* cached_bytes, uint64_t* cap_bytes, int* blocks);
/* th_h5_decode_device keeps per-device scratch memory between calls (compressed span, token arena: ~5 bytes per uncompressed
 * byte of the largest batch so far).  When an allocation fails it frees that scratch and returns TH_ENOMEM — decode fewer
 * datasets per call or read through th_h5_read_chunked_as; th_h5_release_scratch frees it on request (end of a run). */
int th_h5_release_scratch(int device);
/* n independent zlib (wrapped = 1) or raw DEFLATE (wrapped = 0) streams inflated on `device`: stream i is
 * comp[src_off[i] .. + src_len[i]) and decodes to exactly dst_len[i] bytes at out[dst_off[i]] (8-byte aligned).  comp / out are
 * host buffers.  status_out[i] (optional): 0, or why stream i failed (1 input exhausted, 2 output overrun, 3 bad zlib header,
 * 4 invalid code, 5 distance too far back, 6 bad code table, 7 bad stored block, 8 ended short of dst_len, 9 Adler-32 of the
 * output differs from the zlib trailer — what zlib reports as "incorrect data check"; raw streams carry none).  TH_EIO if any failed. */
int th_inflate_many(int device, const void* comp, int64_t comp_len, int64_t n, const int64_t* src_off, const int64_t* src_len,
                    const int64_t* dst_off, const int64_t* dst_len, void* out, int64_t out_len, int wrapped, int* status_out);

/* Resolve MANY datasets' object headers in one call — the per-residue `dataset[pdb][chain][res]` header parse and the
 * two attribute reads of load_batch (`encoded_residue`, utils.py:529) and create_flat_dataset_map (`label`,
 * utils.py:375).  ohdr_addrs[n] are object-header addresses (from the chain groups' symbol tables).  Outputs:
 * btree_out[i] (chunk B-tree address or -1), geom_out[40] (rank, shape[7], chunk[7], element size, datatype class,
 * signed, n_filters, filter ids[8], layout class (1 contiguous: btree_out is then the data address; 2 chunked) of the
 * FIRST dataset), status_out[i] bits: 1 = storage with exactly geom_out's geometry, 2 = numeric attribute `num_attr` copied to num_out[i*num_len ..] as doubles, 4 = string
 * attribute `str_attr` copied NUL-terminated to str_out[i*str_len ..].  Either attribute name may be NULL.  A clear
 * bit means "use the general reader for this one"; nothing is guessed. */
int th_h5_resolve(const void* file, int64_t file_len, int64_t base, int64_t n, const int64_t* ohdr_addrs, const char* num_attr,
                  double* num_out, int num_len, const char* str_attr, char* str_out, int str_len, int64_t* btree_out,
                  int64_t* geom_out, int* status_out, int nthreads);

/* Every link of one old-style HDF5 group in one call (create_flat_dataset_map, reference utils.py:357-375, lists each pdb
 * group, its chain groups and every residue name: `for pdb_code in dataset_file`, `.keys()`).  btree_addr: the group B-tree of
 * the symbol-table message; heap_data / heap_size: absolute offset and length of the local heap's data segment.  names receives
 * the link names, NUL-terminated, in B-tree (name) order — *names_len bytes —, addrs[i] the object-header address of link i,
 * *n_out the count.  TH_ENOMEM: a capacity was too small; TH_EINVAL: not a well-formed group B-tree inside the file. */
int th_h5_group_links(const void* file, int64_t file_len, int64_t base, int64_t btree_addr, int64_t heap_data, int64_t heap_size,
                      char* names, int64_t names_cap, int64_t* addrs, int64_t addrs_cap, int64_t* n_out, int64_t* names_len);

/* ---- voxeliser: the producer of the frames — replaces aposteriori.make_frame_dataset as the reference invokes it
 * (ui.py:73-86: frame_edge_length 21.0, voxels_per_side 21, Codec.CNOCACB, voxels_as_gaussian=True; README.md:83-97).
 * PARITY UNPINNED: aposteriori's source is not in the reference tree; the specification implemented here is written out
 * in timed_hip/voxeliser.py and restated by oracle/voxel_oracle.py.  Host arrays in: atoms_xyz [n_atoms,3] (Angstrom),
 * atom_channel [n_atoms] (index into the atom encoder, < 0 = not encoded), atom_sigma [n_atoms] (Gaussian width in
 * Angstrom; may be NULL for boolean frames), frames_rt [n_res,12] = per residue a row-major 3x3 rotation (rows = local
 * x, y, z axes) followed by the origin (the residue's CA).  Out: [n_res, V, V, V, n_channels], float32 when gaussian
 * else uint8 (0/1); `out` is host memory, or device memory of `device` when out_on_device (frames then go straight to
 * th_predict_device without leaving HBM).  One frame holds at most 2048 encodable atoms (TH_EUNSUP beyond).  An atom
 * whose coordinate in a frame is NaN or infinite is not encoded there: a frames_rt row that holds such a value gives an
 * all-zero frame, never a NaN in the output.
 * This is th_voxelise_batch (below) for ONE structure that owns every atom and every frame, without weights: the same kernel
 * and the same host path.  So the call works on a non-blocking stream of its own and waits for that stream only, never for
 * the whole device.  Every refusal happens before the first HIP call, th_last_error naming th_voxelise: TH_EINVAL for a NULL
 * array where a count is non-zero, a negative count, n_res > INT_MAX (refused, not truncated), voxels_per_side even or
 * > 511, frame_edge_length not positive, Gaussian frames of atoms without sigmas; TH_EUNSUP for n_channels outside 1..8.
 * n_res == 0: TH_OK, nothing is launched.  A failed allocation is TH_ENOMEM when HIP reports out of memory (TH_EHIP
 * otherwise).  When frames overflow the list, the count in th_last_error is the largest over the frames. */
int th_voxelise(int device, const float* atoms_xyz, const int32_t* atom_channel, const float* atom_sigma, int64_t n_atoms,
                const float* frames_rt, int64_t n_res, int voxels_per_side, float frame_edge_length, int n_channels, int gaussian,
                void* out, int out_on_device);

/* ---- batched voxeliser: the frames of many structures in one launch, with an optional weight per atom (the charge / polarity
 * channel of timed_hip/voxeliser.py spec item 8).
 *     *** PARITY UNPINNED AGAINST AMPAL AND APOSTERIORI ***  (the specification is this project's own reading, see voxeliser.py)
 * Arrays as for th_voxelise, the atoms of all structures one after the other: structure s owns the atoms
 * [atom_offsets[s], atom_offsets[s + 1]) (atom_offsets [n_structures + 1], from 0 to n_atoms, never decreasing; a structure may
 * be empty or have no frame).  frames_rt [n_frames, 12] and frame_structure [n_frames]: frame r sees the atoms of structure
 * frame_structure[r] and no others; frames may be listed in any order.  atom_weight [n_atoms] or NULL (every atom counts 1).
 * Rule: frame r is what the specification (timed_hip/voxeliser.py items 3-6 and 8) gives for that structure's atoms alone and
 * that frames_rt row; th_voxelise is the case of one structure.  A Gaussian contribution is acc = acc + weight * (w / total):
 * the quotient, then the product, each rounded to float32, then added, in atom order, no fused multiply-add.  Multiplying by
 * 1.0f is exact, so atom_weight NULL and atom_weight all ones give the same frames byte for byte, and a structure's frames are
 * th_voxelise's byte for byte, Gaussian and boolean alike.  A frame's bytes do not depend on where the frame or its structure sits in the
 * batch or on what else the batch holds (no float atomics).  At most 2048 encodable atoms inside one frame: beyond, the whole
 * call fails with TH_EUNSUP and the count in th_last_error.
 * The call works on a non-blocking stream of its own and waits for that stream only (no device-wide synchronise): a loader thread
 * does not wait for kernels other threads have queued.  The stream is kept for the next call when this one returns (creating one
 * costs milliseconds); calls that overlap hold different streams.  out: host memory, or device memory of `device` when out_on_device (nothing
 * is downloaded then).  kernel_ms (may be NULL): the kernel's time from events on the call's stream.
 * Refused before any HIP call, th_last_error naming th_voxelise_batch — TH_EINVAL: a NULL array where a count is non-zero;
 * atom_offsets[0] != 0, a decreasing offset, a last offset != n_atoms; a frame_structure entry outside [0, n_structures);
 * atom_weight with gaussian == 0 (boolean frames carry no weight); a weight that is not finite; voxels_per_side even or > 511;
 * frame_edge_length not positive.  TH_EUNSUP: n_channels outside 1..8.  n_frames == 0: TH_OK, nothing is launched. */
int th_voxelise_batch(int device, const float* atoms_xyz, const int32_t* atom_channel, const float* atom_sigma,
                      const float* atom_weight, int64_t n_atoms, const int64_t* atom_offsets, int64_t n_structures,
                      const float* frames_rt, const int32_t* frame_structure, int64_t n_frames, int voxels_per_side,
                      float frame_edge_length, int n_channels, int gaussian, void* out, int out_on_device, double* kernel_ms);

/* ---- multi-GPU reassembly (no reference counterpart: the reference is single-process) ----- */
/* one process per GPU; rank 0 creates the id and ships it to the others out of band */
#define TH_COMM_ID_BYTES 128
int th_comm_unique_id(char id[TH_COMM_ID_BYTES]);
int th_comm_init(const char id[TH_COMM_ID_BYTES], int n_ranks, int rank, int device, th_comm** out);
void th_comm_free(th_comm* c);
/* gather contiguous per-rank row shards [counts[r], width] fp32 (device pointers) into
 * d_out [sum(counts), width] on `root` (RCCL send/recv over xGMI; d_out ignored elsewhere) */
int th_comm_gather_rows(th_comm* c, const float* d_local, const int64_t* counts, int width, int root,
                        float* d_out);
int th_comm_barrier(th_comm* c);
/* what this communicator's gathers have issued so far on THIS rank: out = {ncclSend calls, ncclRecv calls, bytes sent, bytes
 * received, device copies of the root's own block}.  A 1-rank gather issues no RCCL transfer (the root's block is a copy) unless
 * TH_COMM_SELF_RCCL=1 was set when th_comm_init ran: then that block goes through a grouped ncclSend/ncclRecv pair to self. */
int th_comm_stats(th_comm* c, int64_t out[5]);

#ifdef __cplusplus
}
#endif
#endif /* TIMED_HIP_H */
