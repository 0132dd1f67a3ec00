/* dasp_hip.h -- C ABI of libdasp_hip.so: the MI355X (gfx950) hot path of dasp_pytorch.functional.
 *
 * Every entry point takes plain device pointers, sizes and a HIP stream (hipStream_t passed as
 * void*; NULL = the null stream). All launches are asynchronous on that stream, out-of-place, and
 * never allocate: the caller owns every buffer (sizes come from the *_floats / *_doubles queries).
 * Return value: 0 = success, >0 = hipError_t of the failed launch, <0 = DASP_ERR_*.
 *
 * The reference (csteinmetz1/dasp-pytorch v0.0.1) has no FFI layer -- its boundary is the Python
 * function API. Each group below names the reference callable (file:line) it replaces; the Python
 * binding that restores the reference signatures is dasp_pytorch_amd/ (see INTEGRATION.md).
 */
#ifndef DASP_HIP_H
#define DASP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Hash of this header as it was when the library was built (csrc/build.py -> csrc/abi.hip). A binding compiled against the header - the
 * torch extension csrc/torch_ext, or a maintainer's own - compares it with the hash it was built with before it trusts the argument lists. */
unsigned long long dasp_abi_hash(void);

#define DASP_OK 0
#define DASP_ERR_ARG (-1)          /* null pointer / inconsistent sizes */
#define DASP_ERR_UNSUPPORTED (-2)  /* e.g. section count without a compiled kernel */
#define DASP_ERR_DEVICE (-3)       /* a kernel of an EARLIER call on this device reported a broken protocol: see dasp_device_error below */

/* ---------------------------------------------------------------------------------------------
 * Device-side errors and the look-back plan.  The segmented launches ("Few rows", "Few batch items") hand segment states between the
 * workgroups of ONE launch as tagged 64-bit words; a reader that waits for a word longer than 2 s of wall clock (a scratch buffer
 * overwritten under the launch, a workgroup that died) stores into a sticky error word of its kernel family and carries on with NaN.
 * The words live in 64 bytes of host-mapped memory per device (one allocation, made by the first call of dasp_device_error() or of a
 * segmented entry point on that device - call dasp_device_error() once before capturing a graph); nothing is copied or polled on the
 * fast path. While a bit is set every segmented entry point returns DASP_ERR_DEVICE instead of launching.
 *   dasp_device_error()        bits of the current device: 1 EQ forward, 2 EQ backward, 4 compressor/expander forward, 8 backward, 16 test,
 *                              32 the random stream's generation kernel (a wave of its pipeline gave up waiting; dasp_mt_randn checks too)
 *   dasp_device_error_clear()  re-arm
 *   dasp_plan_lookback(on)     1 (default): the one-launch look-back forms where they apply; 0: the two-launch forms (pre-pass + pass) -
 *                              no workgroup ever waits for another; < 0: query. Returns the setting.
 * Test support (tests/test_gpu_lookback.py): dasp_test_lookback_timeout(ms) sets the time-out (0 = 2 s); dasp_test_lookback_stall polls a
 * word that never arrives (zero_word: 8 zero bytes on the device; out: 1 float or NULL); dasp_test_spin keeps `workgroups` x `threads`
 * busy for `milliseconds`; dasp_test_stream_with_cus makes a stream confined to the first n_cus compute units (hipExtStreamCreateWithCUMask).
 * ------------------------------------------------------------------------------------------- */
int  dasp_device_error(void);
void dasp_device_error_clear(void);
int  dasp_plan_lookback(int on);
int  dasp_test_lookback_timeout(int milliseconds);
int  dasp_test_lookback_stall(const unsigned long long* zero_word, float* out, void* stream);
int  dasp_test_spin(int workgroups, int threads, double milliseconds, void* stream);
int  dasp_test_stream_with_cus(int n_cus, void** stream);
int  dasp_test_stream_destroy(void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cascaded biquads.  Replaces dasp_pytorch.signal.sosfilt_via_fsm (dasp_pytorch/signal.py:136-166,
 * with fft_sosfreqz :14-32, fft_freqz :7-11, freqdomain_fir :35-39) and, through
 * dasp_peq_prepare, the coefficient design dasp_pytorch.signal.biquad (signal.py:242-306) as used
 * by dasp_pytorch.functional.parametric_eq (dasp_pytorch/functional.py:118-272).
 *
 * x, y, gy, gx: (B, C, N) fp32 contiguous; one filter per batch item shared by its C channels
 * (signal.py:157-158). Bs = number of filter sets: B, or 1 = broadcast over the batch
 * (functional.py:208-220). S = sections per filter; compiled for S in {2,4,6,8}.
 * ------------------------------------------------------------------------------------------- */
int  dasp_sos_supported_sections(int S);          /* 1 if a kernel for S sections is compiled */
int  dasp_sos_chunk(void);                        /* samples per lane chunk (L) */
int  dasp_sos_tile(void);                         /* samples per wave tile (64 L) */
int  dasp_sos_bwd_waves(void);                    /* waves per row in the backward kernel */
long dasp_sos_table_floats(int S);                /* fp32 table size per filter set */
long dasp_sos_dtab_doubles(int S);                /* fp64 side-table size per filter set */
long dasp_sos_num_tiles(long N);
long dasp_sos_carry_floats(long rows, long N, int S);   /* rows = B*C */
long dasp_sos_partial_floats(long rows, int S);          /* scratch between the backward kernel and the finalize step (16-byte aligned; opaque:
                                                          * one 32 x 32 fp64 Gram matrix per row or per (row, segment)) */

/* sos: (Bs, S, 6) fp32, rows [b0 b1 b2 a0 a1 a2] (signal.py:141). Fills tab / dtab. */
int dasp_sos_prepare(const float* sos, int Bs, int S, float* tab, double* dtab, void* stream);

/* params: (Bs, S, 3) fp32 rows [gain_db, cutoff_freq, q_factor]; types[S] (host array):
 * 0 peaking, 1 low_shelf, 2 high_shelf, 3 low_pass, 4 high_pass (signal.py:261-297). */
int dasp_peq_prepare(const float* params, int Bs, int S, const int* types, double sample_rate,
                     float* tab, double* dtab, void* stream);
/* The same from 3*S separate control vectors: rows = host array of device pointers, rows[3*k + c] -> Bs values of control c
 * (0 gain_db, 1 cutoff_freq, 2 q_factor) of section k - the tensors functional.parametric_eq receives (functional.py:118-139). */
int dasp_peq_prepare_rows(const float* const* rows, int Bs, int S, const int* types, double sample_rate, float* tab,
                          double* dtab, void* stream);

/* y = cascade(x). carries (may be NULL when no backward follows) receives the state of every lane chunk
 * (dasp_sos_carry_floats(rows, N, S) floats = 2*S per dasp_sos_chunk() samples, in the kernels' own order); the backward pass reads it
 * instead of re-scanning the forward recurrence. */
int dasp_sosfilt_forward(const float* tab, int Bs, const float* x, float* y, float* carries,
                         int B, int C, long N, int S, void* stream);

/* gx = adjoint cascade(gy) (dasp_sosfilt_backward_ex); partials receives what dasp_sos_grad_finalize_ex turns into the coefficient gradients
 * (per row: the matrix sum over chunks of [gy chunk; adjoint state] [x chunk; forward state]^T, accumulated on the matrix cores:
 * csrc/sosfilt.hip sos_bwd_gram_kernel). dasp_sos_grad_finalize_ex: mode 0: gout (B, S, 6) = dL/dsos;  mode 1: gout (B, S, 3) =
 * dL/d[gain_db, cutoff_freq, q_factor]. With Bs == 1 the caller sums gout over the batch.
 * dasp_sosfilt_backward_grads_ex: the two (same mode / gout) as one call - the autograd of signal.sosfilt_via_fsm
 * (dasp_pytorch/signal.py:136-166) / functional.parametric_eq (functional.py:118-272) in one step. Two launches at one workgroup per row
 * (the segmented forms - dasp_peq_backward - finalize inside their launch and count an item's workgroups in the item's table: hence the
 * non-const tab; the count is left at zero). The _ex suffix of the three is historical: they are the only forms. */

/* The backward pass as asked for (torch.autograd's needs_input_grad) and for the cascade it is:
 *   gx == NULL        no input gradient: the adjoint output is neither transposed back nor stored (parametric_eq is the first effect of
 *                     the reference's chain, examples/style_transfer.py:150 - its input never needs one);
 *   partials == NULL  no coefficient gradients (a fixed filter): x and carries are not read, only the adjoint cascade runs.
 * dasp_sos_grad_finalize_ex: segments = rows of partial sums per (row, wave) (1 after dasp_sosfilt_backward_ex, dasp_sos_segments(N, Tseg)
 * after dasp_sosfilt_backward_seg_ex); mode 2 = mode 1 written as 3*S rows of B values ([3 k + c][item]: one contiguous vector per control tensor). */
int dasp_sosfilt_backward_ex(const float* tab, int Bs, const float* x, const float* gy, const float* carries, float* gx,
                             float* partials, int B, int C, long N, int S, void* stream);
int dasp_sos_grad_finalize_ex(const double* dtab, int Bs, const float* partials, int B, int C, int S, int segments, int mode,
                              float* gout, void* stream);
int dasp_sosfilt_backward_grads_ex(float* tab, const double* dtab, int Bs, const float* x, const float* gy, const float* carries,
                                   float* gx, float* partials, int mode, float* gout, int B, int C, long N, int S, void* stream);

/* functional.parametric_eq (dasp_pytorch/functional.py:118-272) as one call per direction. Forward = dasp_peq_prepare_rows +
 * dasp_sosfilt_forward (Tseg == 0) or + dasp_sos_segment_prepare + dasp_sosfilt_forward_seg (Tseg = dasp_sos_segment_tiles(B*C, N) > 0;
 * segtab / segbuf as below, NULL otherwise). Backward = the adjoint cascade and the control gradients from the tables the forward call
 * filled (designed cascade), gx / partials / mode as above; with Tseg > 0 partials hold dasp_sos_partial_floats(rows * segments, S). */
int dasp_peq_forward(const float* const* rows, int Bp, int S, const int* types, double sample_rate, float* tab, double* dtab,
                     const float* x, float* y, float* carries, int B, int C, long N, long Tseg, double* segtab, float* segbuf,
                     void* stream);
/* The same from the normalised (Bp, 3 S) tensor of Processor.process_normalized (dasp_pytorch/modules.py:25-91) - SURVEY 8(f1)'s fused op:
 * de-normalisation (lo, span: host arrays of 3 S doubles, min and max - min of every column, modules.py:136-155), range check (flag: one
 * device word, zeroed by the caller; bit i is set when column i leaves [0, 1] - read it back to raise the reference's ValueError,
 * modules.py:83-84; NULL = no check), design and cascade. dasp_peq_backward with mode 1 returns the gradient w.r.t. the normalised tensor. */
int dasp_peq_forward_norm(const float* pn, int Bp, int S, const int* types, double sample_rate, const double* lo, const double* span,
                          unsigned* flag, float* tab, double* dtab, const float* x, float* y, float* carries, int B, int C, long N,
                          long Tseg, double* segtab, float* segbuf, void* stream);
int dasp_peq_backward(float* tab, const double* dtab, int Bp, const float* x, const float* gy, const float* carries, float* gx,
                      float* partials, int mode, float* gout, int B, int C, long N, int S, long Tseg, const double* segtab,
                      float* segbuf, void* stream);
/* The design step of dasp_peq_forward_norm on its own: tables from the normalised (Bp, 3 S) tensor, no cascade. Tseg <= 0 and segtab == NULL:
 * tables only; Tseg > 0 (a power of two) with segtab: also the segment transition matrices of dasp_sos_segment_prepare, from the same launch. */
int dasp_peq_prepare_norm(const float* pn, int Bp, int S, const int* types, double sample_rate, const double* lo, const double* span,
                          unsigned* flag, float* tab, double* dtab, long Tseg, double* segtab, void* stream);
/* The first two launches of dasp_sosfilt_forward_seg on their own (scan-only pre-pass + chain): afterwards the second half of segbuf
 * (dasp_sos_seg_floats floats) holds the state every (row, segment) starts from, [row][segment][2 S]. */
int dasp_sos_segment_starts(const float* tab, const double* segtab, int Bs, const float* x, float* segbuf, int B, int C, long N, int S,
                            long Tseg, void* stream);

/* ---- fused forward of the reference's effect chain: parametric EQ -> compressor -----------------------------------------------------------
 * examples/style_transfer.py:150-154 (equalizer -> compressor -> reverb -> gain) and :293-299 (the same chain without gradients, every
 * training step, to synthesise the target). y = compressor(parametric_eq(x)) in ONE pass over x: a workgroup owns a batch item (both
 * channels: the compressor's side chain is their sum, functional.py:328), a tile of the EQ's output goes through the gain computer, the
 * one-pole smoothing scan and the output multiply before it leaves the chip. 8 B per channel-sample instead of 16 for the two separate
 * forward calls; forward only (no chunk states or carries are saved). The chain's final gain commutes with the reverb and is folded
 * into makeup_gain_db by the caller (dasp_chain_controls).
 *   tab  : the EQ's tables (dasp_peq_prepare / _rows / _norm; Bs = 1 or B items; S = 6)      ctl : (B, 5) as for dasp_dynamics_forward
 *   mode : 0 compressor, 1 expander; no look-ahead                                            x, y: (B, C, N), C = 1 or 2
 *   Tseg : 0 = one workgroup per item, or dasp_chain_segment_tiles(B, N) (few items: every item cut into segments of Tseg tiles) with
 *          segtab from dasp_sos_segment_prepare(dtab, Bs, S, Tseg, ...) and segbuf of dasp_chain_seg_floats(B, C, N, S, Tseg) floats */
long dasp_chain_segment_tiles(long B, long N);
long dasp_chain_seg_floats(long B, long C, long N, int S, long Tseg);
int dasp_chain_forward(const float* tab, int Bs, const float* x, const float* ctl, float* y, int B, int C, long N, int S, int mode,
                       double sample_rate, float eps, long Tseg, const double* segtab, float* segbuf, void* stream);
/* The same pass for the step that carries gradients: also writes the EQ's output yeq (B, C, N) - the input of dasp_dynamics_backward -, the
 * EQ's chunk start states eq_carries (dasp_sos_carry_floats(B * C, N, S) floats, for dasp_peq_backward / dasp_sosfilt_backward_ex) and the
 * smoothing state entering every compressor tile dyn_carries (dasp_dyn_carry_floats(B, N) floats): 15 B per channel-sample instead of 19
 * for the two forward calls. One workgroup per item (no segments); pays from ~200 items on (profiles/r06/chain_fwd_saving_ab.log). */
int dasp_chain_forward_saving(const float* tab, int Bs, const float* x, const float* ctl, float* y, float* yeq, float* eq_carries,
                              float* dyn_carries, int B, int C, long N, int S, int mode, double sample_rate, float eps, void* stream);

/* dasp_pytorch.signal.biquad (dasp_pytorch/signal.py:242-306) as a call of its own: the fp64 RBJ design the prepare calls run, for n
 * (gain_db, cutoff_freq, q_factor) triples of one filter type. ba: (n, 6) fp64 rows [b0 b1 b2 1 a1 a2] (normalised by a0, as the
 * reference returns them); jac: (n, 15) fp64 = d(b0 b1 b2 a1 a2)/d(gain_db, cutoff_freq, q_factor), which dasp_biquad_backward
 * contracts with gba (n, 6), the gradient w.r.t. the rows of ba, into gparams (n, 3). */
int dasp_biquad_design(const double* gain_db, const double* cutoff_freq, const double* q_factor, int n, int type,
                       double sample_rate, double* ba, double* jac, void* stream);
int dasp_biquad_backward(const double* jac, const double* gba, int n, double* gparams, void* stream);

/* Few rows (B*C <= 128; from there up to 256 rows the plain calls launch twice the waves per row instead): a row is one workgroup, so the calls above
 * would leave most of the chip idle. The *_seg entry points cut every row into segments of Tseg tiles that run as independent workgroups;
 * same results (oracle/chunkscan_model.py forward_row_segmented / backward_row_segmented).
 *   dasp_sosfilt_forward_seg / dasp_sosfilt_backward_seg_ex (tables that may serve many calls): per direction a scan-only pre-pass gives
 *     every segment's end state, the last of an item's workgroups to finish chains them through Phi^(samples per segment)
 *     (dasp_sos_segment_prepare, from dtab; the completion counters are words of the item's table, zeroed by the prepare call and reset
 *     after use - the one place where a call writes into `tab`), then the ordinary pass runs per segment from its start state.
 *   dasp_peq_forward* / dasp_peq_backward (a design launch per call): ONE launch per direction - every workgroup sweeps its segment
 *     scan-only, hands the end state on as tagged 64-bit words in segbuf (8-byte aligned) and takes its start state from the words of the
 *     row's other segments (a decoupled look-back; the tag is drawn by the call's design launch, so dasp_peq_backward needs tables filled
 *     by dasp_peq_forward* of the same step), then runs the pass; the backward launch also finalizes the control gradients. Three
 *     launches per step: design, forward, backward.
 *   Tseg   = dasp_sos_segment_tiles(rows, N): proposed tiles per segment (a power of two), 0 = use the plain calls
 *   segtab = dasp_sos_segtab_doubles(S) doubles per item (Bs items): the two segment transition matrices + the basis responses of the Gram
 *            finalize step (filled by the design launch of dasp_peq_forward*);  segbuf = dasp_sos_seg_floats(rows, N, S, Tseg) floats of scratch
 *   partials of the backward pass: dasp_sos_partial_floats(rows * dasp_sos_segments(N, Tseg), S) floats, finalized by
 *   dasp_sos_grad_finalize_ex(..., segments = dasp_sos_segments(N, Tseg), ...) after dasp_sosfilt_backward_seg_ex. */
long dasp_sos_segment_tiles(long rows, long N);
long dasp_sos_segments(long N, long Tseg);
long dasp_sos_segtab_doubles(int S);
long dasp_sos_seg_floats(long rows, long N, int S, long Tseg);
int dasp_sos_segment_prepare(const double* dtab, int Bs, int S, long Tseg, double* segtab, void* stream);
int dasp_sosfilt_forward_seg(const float* tab, const double* segtab, int Bs, const float* x, float* y, float* carries,
                             float* segbuf, int B, int C, long N, int S, long Tseg, void* stream);
int dasp_sosfilt_backward_seg_ex(const float* tab, const double* segtab, int Bs, const float* x, const float* gy,
                                 const float* carries, float* gx, float* partials, float* segbuf,
                                 int B, int C, long N, int S, long Tseg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * gain / distortion.  Replace dasp_pytorch.functional.gain (dasp_pytorch/functional.py:10-29):
 * y = x * 10^(gain_db/20), gain_db (B) one value per batch item repeated over channels (:26-28);
 * and dasp_pytorch.functional.distortion (functional.py:65-78): y = tanh(x * 10^(drive_db/20)),
 * drive_db (B*C) one value per (b, c) row (the reference's drive_db.view(bs, chs, -1), :78).
 * Backward: gx = dL/dx, ggain (B) / gdrive (B*C) = dL/d(control in dB); `partials` is scratch of
 * dasp_ew_partial_floats(B*C, N) floats.
 * ------------------------------------------------------------------------------------------- */
long dasp_ew_partial_floats(long rows, long N);
int dasp_gain_forward(const float* x, const float* gain_db, float* y, int B, int C, long N, void* stream);
int dasp_gain_backward(const float* x, const float* gain_db, const float* gy, float* gx, float* ggain,
                       float* partials, int B, int C, long N, void* stream);
int dasp_distortion_forward(const float* x, const float* drive_db, float* y, int B, int C, long N, void* stream);
int dasp_distortion_backward(const float* x, const float* drive_db, const float* gy, float* gx, float* gdrive,
                             float* partials, int B, int C, long N, void* stream);
/* distortion with one drive value per SAMPLE: the reference's drive_db.view(bs, chs, -1) also takes bs * chs * seq_len values
 * (functional.py:78). x, drive_db, y, gy, gx, gdrive: n = B * C * N floats each; gdrive = dL/d(drive_db) per sample. */
int dasp_distortion_sample_forward(const float* x, const float* drive_db, float* y, long n, void* stream);
int dasp_distortion_sample_backward(const float* x, const float* drive_db, const float* gy, float* gx, float* gdrive, long n, void* stream);

/* Controls of the reference's effect chain (examples/style_transfer.py:150-154: equalizer -> compressor -> reverb -> gain, each through
 * Processor.process_normalized, dasp_pytorch/modules.py:25-51) from the normalised parameter tensors in one launch: comp_pn (B, 6),
 * reverb_pn (B, 25), gain_pn (B, 1) in [0, 1]; lo, span: HOST arrays of 32 floats, [0, 6) the compressor's ranges in the order of its
 * param_ranges (modules.py:159-187), [6, 31) the reverb's, [31] the gain's. Out: ctl (B, 5) as dasp_dynamics_forward takes it, with the
 * gain added to the make-up gain (a per-item gain commutes with the linear reverb); gains, decays (B, 12), mix (B) as
 * dasp_reverb_forward takes them. The backward call maps the gradients of those four back to the three parameter tensors. */
/* flag (may be NULL): one device word; bit i is OR-ed in when column i of the 32 (compressor 0-5, reverb 6-30, gain 31) holds a value outside
 * [0, 1] (the reference's ValueError, modules.py:83-84: the host reads the word back when it chooses to; it is never cleared here). */
int dasp_chain_controls(const float* comp_pn, const float* reverb_pn, const float* gain_pn, const float* lo, const float* span, float* ctl,
                        float* gains, float* decays, float* mix, unsigned* flag, int B, void* stream);
int dasp_chain_controls_backward(const float* gctl, const float* ggain, const float* gdecay, const float* gmix, const float* span,
                                 float* gcomp_pn, float* greverb_pn, float* ggain_pn, int B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dynamics: compressor / expander.  mode 0 replaces dasp_pytorch.functional.compressor
 * (dasp_pytorch/functional.py:275-399: side-chain sum :328, level in dB :347, soft-knee gain
 * computer :350-369, one-pole smoothing :372-380 which the reference evaluates through
 * signal.lfilter_via_fsm, dasp_pytorch/signal.py:95-133, look-ahead delay :383-385, make-up and
 * dB->linear :388-394). mode 1 is a downward expander of the same structure; the reference's
 * expander is a stub (functional.py:402-403), so it has no reference behaviour.
 *
 * x, y, gy, gx: (B, C, N) fp32 contiguous. ctl: (B, 5) fp32 rows [threshold_db, ratio, attack_ms,
 * knee_db, makeup_gain_db] (release_ms is unused by the reference, :340,343-344, and has no entry).
 * carries: dasp_dyn_carry_floats(B, N) floats written by forward, read by backward (may be NULL in
 * forward when no backward follows). lin_buf: (B, N) floats, required only when lookahead > 0
 * (forward writes the linear gain, backward reads it at shifted positions). gctl: (B, 5) = dL/dctl.
 * partials: scratch of dasp_dyn_partial_floats(B) floats.
 * ------------------------------------------------------------------------------------------- */
long dasp_dyn_num_tiles(long N);
long dasp_dyn_carry_floats(long B, long N);
long dasp_dyn_partial_floats(long B);
int dasp_dyn_counters_reset(int* counters, int B, void* stream);
/* Few batch items (B < 128; the reference trains with 8 to 32: examples/style_transfer.py:403, auto_eq.py:231): one workgroup per item
 * would leave most of the chip idle, so every item can be cut into segments of Tseg tiles that run as independent workgroups - scan-only
 * pre-pass, a scalar chain through alpha^(samples per segment) in fp64, then the ordinary pass per segment; same results.
 *   Tseg = dasp_dyn_segment_tiles(B, N) (a power of two); Tseg <= 0 = one workgroup per item: segbuf and counters are then unused and may
 *   be NULL, partials as above. Tseg > 0: segbuf = 2 * B * dasp_dyn_segments(N, Tseg) floats of scratch; carries as above; partials of the
 *   backward pass: dasp_dyn_partial_floats(B * dasp_dyn_segments(N, Tseg)) floats; counters: below. */
long dasp_dyn_segment_tiles(long B, long N);
long dasp_dyn_segments(long N, long Tseg);
int dasp_dynamics_forward(int mode, const float* x, const float* ctl, float* y, float* carries, float* lin_buf, float* segbuf,
                          int B, int C, long N, double sample_rate, float eps, int lookahead, long Tseg, int* counters, void* stream);
int dasp_dynamics_backward(int mode, const float* x, const float* ctl, const float* gy, const float* carries,
                           const float* lin_buf, float* gx, float* gctl, float* partials, float* segbuf, int B, int C, long N,
                           double sample_rate, float eps, int lookahead, long Tseg, int* counters, void* stream);
/* functional.compressor / expander on the reference's own six control tensors (dasp_pytorch/functional.py:275-286), without a stacking
 * launch in front of the kernels or a transposition behind them: rows = 5 device vectors of B floats (threshold_db, ratio, attack_ms,
 * knee_db, makeup_gain_db; the array of pointers itself is host memory), grows = 6 device vectors of B floats that receive the gradients
 * in the reference's argument order (threshold_db, ratio, attack_ms, release_ms - set to zero: it has no path to the output,
 * functional.py:340,343-344 -, knee_db, makeup_gain_db). Everything else, Tseg, segbuf and counters included, as dasp_dynamics_forward /
 * _backward. */
int dasp_dynamics_forward_rows(int mode, const float* x, const float* const* rows, float* y, float* carries, float* lin_buf, float* segbuf,
                               int B, int C, long N, double sample_rate, float eps, int lookahead, long Tseg, int* counters, void* stream);
int dasp_dynamics_backward_rows(int mode, const float* x, const float* const* rows, const float* gy, const float* carries,
                                const float* lin_buf, float* gx, float* const* grows, float* partials, float* segbuf, int B, int C, long N,
                                double sample_rate, float eps, int lookahead, long Tseg, int* counters, void* stream);
/* counters (may be NULL): a buffer of AT LEAST 4 * B ints owned by the caller, one buffer per stream, ZERO before its first use; every
 * call returns the words it used to zero. dasp_dyn_counters_reset(counters, B, stream) zeroes them on the stream (a kernel): call it after
 * allocating the buffer and after any segmented call that returned an error - a launch that did not complete may leave a count behind,
 * and a count that never completes means wrong start states and gradients for every later call (both bindings of this repo drop their
 * cached buffer when a call fails). (Rounds 3 - 4 zeroed them with hipMemsetAsync at the start of every call; inside a captured
 * graph that memset node was not ordered before the kernel behind it when a replay started on an idle device, so the library zeroes
 * nothing with memset nodes any more - csrc/common.hpp zero_async.) With them the forward pass is ONE launch when Tseg is 1, 2 or 4
 * tiles per forward wave (16, 32, 64: every workgroup runs its segment from a zero state, hands the segment's end state on as a tagged
 * 64-bit word in segbuf - 8-byte aligned - and corrects its tile carries by the look-back sum over the item's earlier segments; the
 * smoothing state is one float that enters linearly) and the backward pass is one launch when Tseg is two tiles per backward wave (16)
 * with lookahead 0, C <= 2 and 16-byte aligned rows; otherwise the item's last workgroup of a pre-pass chains the segments and the last
 * one of the adjoint pass forms the control gradients: two launches per direction instead of three / four (workgroup to workgroup by
 * agent-scope atomics, csrc/common.hpp handoff_arrive_is_last, as for the biquad cascade). */

/* ---------------------------------------------------------------------------------------------
 * Noise-shaped reverberation.  Replaces dasp_pytorch.functional.noise_shaped_reverberation
 * (dasp_pytorch/functional.py:406-577): grouped FIR filter bank over white noise (:548-558),
 * per-band exponential envelope x gain and mean over bands (:561-567), causal convolution of the
 * input with the resulting 2-channel impulse response truncated to N (:570-572), wet/dry mix (:575).
 * The filter design (dasp_pytorch.signal.octave_band_filterbank, dasp_pytorch/signal.py:42-92,
 * SciPy firwin on the host) stays on the host; its taps are passed in.
 *
 * Both convolutions run on the library's own register/LDS FFTs (no FFT library is linked or loaded): the filter
 * bank (taps <= 3585) as one fused kernel that is re-run in the backward pass instead of saving its output, the
 * long convolution (L <= 2^20) as overlap-add with four-step transforms of pairs of blocks (reverb.hip).
 *
 * x, y, gy, gx: (B, 2, N) fp32.  noise: (2B, nb, L + taps - 1).  gains, decays: (B, nb).  mix: (B).
 * nb <= 16 bands, L = IR length, taps = FIR length.  All buffer sizes come from dasp_reverb_sizes.
 * ------------------------------------------------------------------------------------------- */
/* Plan overrides of the reverb - explicit arguments for the three choices its planner makes (rounds 2 - 4 read them from the environment;
 * a library should not): chunk = signals per pass of the long-convolution pipeline (<= 0: all at once, the default), weight_limit = largest
 * |rho| * 4096 served with the envelope inside the filter bank's transform (0: every item the per-band way; < 0: the default),
 * band_split = workgroups per (item, window) of the filter bank (< 1: the planner's rule). Process-wide: set before dasp_reverb_sizes and
 * the calls that use its numbers, set back to (-1, -1, -1) afterwards. Developer A/Bs and the tests of the alternative routes. */
int dasp_reverb_plan(long chunk, float weight_limit, int band_split);

/* sizes[0] = block length Lb, [1] = transform length n1, [2] = pairs of blocks per signal, [3] = blocks per signal,
 * [4] = complex (2 x fp32) elements of Fspec, [5] = filter-bank windows per batch item,
 * [6] = complex elements of A (2B * pairs * n1), [7] = complex elements of H (B * n1: the two impulse responses of an item are one complex
 *       frame, left + i right), [8] = floats of each of ir / gir,
 * [9] = signals per pass of the long-convolution pipeline (all 2B by default; a developer switch can cut the pipeline into passes over
 *       chunks of signals that reuse chunk-sized scratch buffers),
 * [10] = floats of mix_part, [11] = floats of part,
 * [12] = complex elements of each of the scratch buffers W / W2 / Ag (at least B * nb * 4096: W and Ag also hold the per-item weighted
 *        band spectra of the filter bank while it runs), [13] = complex elements of each of the scratch buffers Ah / P. */
int dasp_reverb_sizes(int B, long N, int L, int taps, int nb, long* sizes /* [14] */);
/* filters (nb, taps) fp32, the host-designed bank -> Fspec: transform twiddles, the band spectra, the taps themselves (the filter bank
 * re-weights them by each item's decay envelope per call). */
int dasp_reverb_filter_spectrum(const float* filters, int nb, int taps, void* Fspec, void* stream);
/* forward: H, ir (the impulse responses) and (when a backward pass follows) A are kept for it - pass A = NULL otherwise and the column
 * transforms of x go to the scratch W2; W, Ah are scratch.
 * backward: takes the forward call's ir (first argument), H and A - not x; gx, ggain (B, nb), gdecay (B, nb), gmix (B) are the results;
 * Ag, W, P, gir, part, mix_part are scratch. Neither the wet signal nor x is needed for d loss / d mix = sum_n gy (wet - x):
 * sum_n gy wet = sum_r ir[r] c[r] and sum_n gy x = c[0] with c[r] = sum_n gy[n] x[n - r], r < L - the correlation the pass forms for
 * d loss / d ir anyway. */
int dasp_reverb_forward(const float* x, const float* noise, unsigned long long seed, const unsigned long long* seed_dev, const void* Fspec,
                        const float* gains, const float* decays, const float* mix, float* y, void* A, void* H, void* W, void* W2, void* Ah,
                        float* ir, int B, int Cx, long N, int L, int taps, int nb, float decay_bound, void* stream);
int dasp_reverb_backward(const float* ir, const float* gy, const float* noise, unsigned long long seed, const unsigned long long* seed_dev,
                         const void* Fspec, const float* gains, const float* decays, const float* mix, const void* A, const void* H,
                         float* gx, float* ggain, float* gdecay, float* gmix, void* Ag, void* W, void* P, float* gir, float* part,
                         float* mix_part, int B, int Cx, long N, int L, int taps, int nb, float decay_bound, void* stream);
/* Cx: channels of x, 2, or 1 for a mono input (the reference duplicates it to stereo, functional.py:493-495: here both output channels read
 * the one row - no copy; gx stays (B, 2, N), the gradient w.r.t. the mono input is the sum of its two rows).
 * decay_bound: > 0 = the caller vouches that no band decay exceeds this value (Processor.process_normalized: the validated upper end of the
 * parameter range); when even that decay stays on the envelope-inside-the-transform route of the filter bank, the other route's (empty) launch
 * is skipped. 0 = unknown.
 * noise != NULL: the white noise of functional.py:548 is read from memory; seed and seed_dev are ignored. noise == NULL: it is generated
 * inside the filter-bank kernels from the 64-bit seed (the `device_noise=True` mode of the Python layer): a counter-based stream, a pure function of (seed, batch item, band,
 * sample index) - one 32-bit hash per (item, band, index), its halves a Box-Muller pair = the item's two noise rows - so the forward and
 * the backward pass recompute identical values and nothing of size (2B, nb, L + taps - 1) exists (0.82 GB at B = 128 and the default
 * sizes, which torch.randn wrote once and the two filter-bank kernels read once each). Both calls of a step take the same seed.
 * seed_dev (may be NULL): one 64-bit device word added to `seed` when the kernels run - a launch captured into a HIP graph has its by-value
 * seed frozen; bumping the word between replays gives every replay new noise.
 * dasp_reverb_noise writes the stream out in the reference's layout, out (2B, nb, row_len), row_len = L + taps - 1 < 2^24: a test hook
 * (the calls above, given that tensor as noise, must reproduce the seeded calls). Specification: oracle/noise_stream.py. */
int dasp_reverb_noise(unsigned long long seed, const unsigned long long* seed_dev, float* out, int B, int nb, long row_len, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stereo utilities.  Replace dasp_pytorch.functional.stereo_widener (dasp_pytorch/functional.py:580-605),
 * stereo_panner (:608-636) and stereo_bus (:32-62).
 *   widener: x, y (B, 2, N); width (B).            left = L + (1 - 2 width) R, right = (1 - 2 width) L + R
 *   panner:  x (B, T, N); pan (B * T); y (B, 2, T, N).  y[:, 0] = lg x, y[:, 1] = rg x, constant-power-like gains of pan
 *   bus:     x (B, 2, T, N); send_db (B * T); y (B, 2, N).  y = sum over tracks of 10^(send_db / 20) x;  T <= 64
 * partials: dasp_stereo_partial_floats(op, B, T, N) floats (op 0 widener, 1 panner, 2 bus).
 * ------------------------------------------------------------------------------------------- */
long dasp_stereo_partial_floats(int op, long B, int T, long N);
int dasp_widener_forward(const float* x, const float* width, float* y, int B, long N, void* stream);
int dasp_widener_backward(const float* x, const float* width, const float* gy, float* gx, float* gwidth, float* partials, int B,
                          long N, void* stream);
int dasp_panner_forward(const float* x, const float* pan, float* y, int B, int T, long N, void* stream);
int dasp_panner_backward(const float* x, const float* pan, const float* gy, float* gx, float* gpan, float* partials, int B, int T,
                         long N, void* stream);
int dasp_bus_forward(const float* x, const float* send_db, float* y, int B, int T, long N, void* stream);
int dasp_bus_backward(const float* x, const float* send_db, const float* gy, float* gx, float* gsend, float* partials, int B, int T,
                      long N, void* stream);
/* stereo_mix: fader, pan and bus sum of T mono tracks in one pass - what dasp_bus_forward(dasp_panner_forward(x, pan), gain_db) computes,
 * without the (B, 2, T, N) tensor between them - and, optionally, a post-fader, post-pan effects send (a second bus).
 *   x (B, T, N); gain_db, pan, send_db (B * T); mix, send (B, 2, N).   g = 10^(gain_db / 20), s = 10^(send_db / 20), l, r the panner's gains
 *   mix[b, 0] = sum_t g l x[b, t],  mix[b, 1] = sum_t g r x[b, t],  send[b, c] = the same sums with s g in place of g
 * send_db and send (forward), send_db, gsend and gsend_db (backward) are given together or are all NULL (no send bus): anything else, a
 * null pointer elsewhere or a non-positive size is DASP_ERR_ARG. gx may be NULL (x needs no gradient: it is neither computed nor written).
 * T <= dasp_stereo_mix_max_tracks() (256) and B * ceil(N / segment) < 2^31, else DASP_ERR_UNSUPPORTED; all of it is checked before any launch.
 *   dasp_stereo_mix_segment(B, N): samples per workgroup - 4096, halved down to 1024 while B * ceil(N / segment) is below 512 workgroups
 *     (two per compute unit). It fixes the layout of partials (B, segments, T, 2 or 4) and nothing else: what is computed for a sample of
 *     mix, send or gx does not depend on it.
 *   partials: dasp_stereo_mix_partial_floats(B, T, N, with_send) floats of scratch for the backward call (two launches, no atomics:
 *     results are bit-identical run to run).
 *   Non-finite input: a NaN or +-inf sample of a track reaches that sample of both channels of its item's mix and send - through a
 *     muted (gain_db = -inf) or hard-panned track too: 0 x NaN - and nothing else there; gx does not depend on x; that track's three
 *     control gradients are non-finite and no other's. A NaN control makes the item's buses, that track's gx and its control gradients
 *     NaN (a NaN pan is not read as a hard pan, whose vanishing term is dropped). Other items keep every bit. */
int dasp_stereo_mix_segment(long B, long N);
int dasp_stereo_mix_max_tracks(void);
long dasp_stereo_mix_partial_floats(long B, int T, long N, int with_send);
int dasp_stereo_mix_forward(const float* x, const float* gain_db, const float* pan, const float* send_db, float* mix, float* send, int B,
                            int T, long N, void* stream);
int dasp_stereo_mix_backward(const float* x, const float* gain_db, const float* pan, const float* send_db, const float* gmix,
                             const float* gsend, float* gx, float* ggain, float* gpan, float* gsend_db, float* partials, int B, int T,
                             long N, void* stream);

/* oversampled_distortion: tanh(g x) at L times the sample rate, g = 10^(drive_db / 20) - interpolation by L with a windowed-sinc low-pass,
 * the non-linearity, the same low-pass and decimation by L, in one kernel per direction (csrc/oversample.hip); the L-times-longer signal
 * exists in LDS only.  x, y, gy, gx (B, C, N) fp32; drive_db, gdrive (B * C), one value per row; taps: 2 H L + 1 HOST floats h[c],
 * c = -H L .. H L, symmetric (dasp_pytorch_amd.signal.oversampling_taps), handed to the kernels by value.  Zeros outside [0, N):
 *   u[m] = sum_j h[m - L j] x[j],  v[m] = tanh(g u[m]) for 0 <= m < L N (zero outside),  y[n] = (1 / L) sum_m h[L n - m] v[m]
 * Backward: gx = dL/dx and gdrive = dL/d(drive_db), u recomputed; partials is scratch of dasp_osdist_partial_floats(B * C, N, L) floats =
 * rows * ceil(N / dasp_osdist_tile(L)), one per workgroup, summed in fp64 by a second launch: no atomics, bit-identical run to run.
 * L one of 2, 4, 8 and 1 <= H <= 16; anything else, a null pointer or a non-positive size: DASP_ERR_ARG (-1 from the size queries);
 * B * C * ceil(N / tile) >= 2^31: DASP_ERR_UNSUPPORTED. All of it is checked before taps is read and before any launch.
 * Non-finite input: a NaN sample x[j] (or gy[j]) makes y and gx (gx) NaN on [j - 2 H, j + 2 H] of its row and nowhere else, and gdrive
 * of the row NaN. A +-inf or huge sample saturates tanh: y and gx stay finite everywhere (the zeros that pad the taps to whole rows of L
 * are never multiplied - 0 x inf); gdrive of the row is NaN for +-inf (0 x inf in sum s u) and finite for a huge finite sample. A NaN
 * drive_db makes its row NaN. Other rows keep every bit. */
int dasp_osdist_tile(int L);
long dasp_osdist_partial_floats(long rows, long N, int L);
int dasp_osdist_forward(const float* x, const float* drive_db, const float* taps, float* y, int B, int C, long N, int L, int H, void* stream);
int dasp_osdist_backward(const float* x, const float* drive_db, const float* taps, const float* gy, float* gx, float* gdrive, float* partials,
                         int B, int C, long N, int L, int H, void* stream);

/* modulated_delay: chorus / flanger / vibrato - V voices of a delay line whose length a sine LFO moves, read with Catmull-Rom
 * interpolation and mixed with the dry signal, one kernel per direction (csrc/moddelay.hip).  x, y, gy, gx (B, C, N) fp32; ctl, gctl
 * (B, V, 4) fp32, per voice (delay_ms, depth_ms, rate_hz, phase in turns); mix, gmix (B).  For item b, voice v, channel c, sample n, with x
 * zero outside [0, N):
 *   theta = 2 pi (rate_hz n / sample_rate + phase + c stereo_spread)
 *   d = clamp(sample_rate/1000 (delay_ms + depth_ms sin theta), 0, sample_rate/1000 max_delay_ms),  p = n - d,  i = floor(p),  f = p - i
 *   tap_v[n] = sum_{k = -1 .. 2} w_k(f) x[i + k]  (Catmull-Rom),   y[n] = (1 - mix) x[n] + (mix / V) sum_v tap_v[n]
 * theta, d, p and i are float64 in the kernels; f is rounded to float32 and everything after it is float32. For d < 1 the footprint
 * reaches x[n + 1].
 * H: a whole number of samples with sample_rate/1000 max_delay_ms <= H <= dasp_moddelay_max_delay_samples(); it sets the staged window
 * and the tile, dasp_moddelay_tile(H) samples per workgroup.  1 <= V <= dasp_moddelay_max_voices().
 * Backward: gx (NULL: not computed), gctl and gmix, x's taps recomputed; partials is scratch of
 * dasp_moddelay_partial_floats(B * C, N, V, H) = rows * ceil(N / tile) * (4 V + 1) floats, summed in fp64 in a fixed order by a second
 * launch. No global atomics. y, gctl and gmix are bit-identical run to run; gx is accumulated with LDS float adds whose order varies:
 * equal to rounding. The delay gradients take no contribution from samples where d was clamped.
 * A null pointer (gx apart), a non-positive size, V < 1, H < 1, H below the largest delay, a sample rate that is not positive or a
 * non-finite max_delay_ms / stereo_spread: DASP_ERR_ARG (-1 from the size queries); V or H above its maximum, or
 * B * C * ceil(N / tile) >= 2^31: DASP_ERR_UNSUPPORTED (-2 from the size queries). All of it is checked before any launch.
 * Non-finite input: all four products of a tap are always formed, and so is the dry term - a NaN or inf sample under a zero weight
 * gives NaN. A control that makes p NaN reads at i = n (nothing out of range) with f = NaN: the item's y, gx, gmix and that voice's
 * gradients are NaN.
 * Other items keep every bit. */
int dasp_moddelay_max_voices(void);
int dasp_moddelay_max_delay_samples(void);
int dasp_moddelay_tile(int H);
long dasp_moddelay_partial_floats(long rows, long N, int V, int H);
int dasp_moddelay_forward(const float* x, const float* ctl, const float* mix, float* y, int B, int C, long N, int V, int H, double sample_rate,
                          double max_delay_ms, double stereo_spread, void* stream);
int dasp_moddelay_backward(const float* x, const float* ctl, const float* mix, const float* gy, float* gx, float* gctl, float* gmix,
                           float* partials, int B, int C, long N, int V, int H, double sample_rate, double max_delay_ms, double stereo_spread,
                           void* stream);

/* feedback_delay: echo / slap-back / comb - one delay line read with Catmull-Rom interpolation and fed back into itself through a
 * one-pole low-pass, mixed with the dry signal; a recurrence evaluated in place, one workgroup per (b, c) row (csrc/fbdelay.hip).
 * x, y, v, gy, gx (B, C, N) fp32; ctl, gctl (B, 4) fp32: delay_ms, feedback, damping_hz, mix.  For item b, every channel, sample n, with
 * v zero before sample 0:
 *   D = clamp(sample_rate/1000 delay_ms, 2, sample_rate/1000 max_delay_ms),  i = floor(D),  f = D - i
 *   a = exp(-2 pi max(damping_hz, 0) / sample_rate)                                   (damping_hz = +inf: a = 0, no filter)
 *   r[n] = sum_{k = -1 .. 2} w_k(f) v[n - i - k]  (Catmull-Rom),   w[n] = x[n] + feedback r[n],   v[n] = (1 - a) w[n] + a v[n - 1]
 *   y[n] = (1 - mix) x[n] + mix r[n]
 * D, i and a are float64 in the kernels; f and a are rounded to float32 and everything after them is float32. feedback is not clamped.
 * H: a whole number of samples with 2 <= sample_rate/1000 max_delay_ms <= H <= dasp_fbdelay_max_delay_samples(); it sets the ring of
 * LDS that holds the line. A row is walked in sequential steps of dasp_fbdelay_block(H, i - 1) = min(i - 1, 2048) samples.
 * Forward: v (NULL: not saved) is the line's input, which the backward pass reads.  Backward: gx (NULL: not written), gctl; r, w and
 * the derivative taps are recomputed from v; partials is scratch of dasp_fbdelay_partial_floats(B * C, N, H) = 4 floats per row,
 * summed over an item's channels in fp64 in a fixed order by a second launch. No atomics. y, v, gx and gctl are bit-identical run to
 * run. The delay_ms gradient is zero where D was clamped, the damping_hz gradient zero where damping_hz < 0 and at +inf.
 * dasp_fbdelay_prepare() raises the kernels' dynamic-LDS limit on the current device; the binding calls it once when it loads the
 * library, and the first call on a device that was not prepared does it itself.
 * A null pointer (v in forward and gx apart), a non-positive size, H < 2, sample_rate/1000 max_delay_ms below 2 or above H, a sample rate
 * that is not positive and finite, a lag outside [1, H - 1]: DASP_ERR_ARG (-1 from the queries); H above its maximum or B * C >= 2^31:
 * DASP_ERR_UNSUPPORTED (-2 from the queries). All of it is checked before any launch.
 * Non-finite input: all four products of a tap are always formed - a NaN or inf under a zero weight gives NaN - and a NaN or inf
 * sample stays in the line from then on. A NaN delay_ms reads at i = 2 (nothing out of range) with f = NaN: the item's y, gx and
 * control gradients are NaN; an infinite one is clamped. Other items keep every bit. */
int dasp_fbdelay_max_delay_samples(void);
int dasp_fbdelay_block(int H, long lag);
long dasp_fbdelay_partial_floats(long rows, long N, int H);
int dasp_fbdelay_prepare(void);
int dasp_fbdelay_forward(const float* x, const float* ctl, float* y, float* v, int B, int C, long N, int H, double sample_rate,
                         double max_delay_ms, void* stream);
int dasp_fbdelay_backward(const float* x, const float* ctl, const float* v, const float* gy, float* gx, float* gctl, float* partials, int B,
                          int C, long N, int H, double sample_rate, double max_delay_ms, void* stream);

/* fdn_reverb: feedback delay network - K delay lines of whole lengths coupled through the Householder matrix I - (2/K) 1 1^T, each fed
 * through a one-pole low-pass, mixed with the dry signal; a recurrence evaluated in place, one workgroup per (b, c) row (csrc/fdn.hip).
 * x, y, gy, gx (B, C, N) fp32; v (B, C, K, N) fp32; ctl, gctl (B, 3) fp32: decay_s, damping_hz, mix. delays: K ints in HOST memory, the
 * line lengths m_k >= 1 in samples (repeats allowed), read before the call returns. decorrelate: 0 or 1.  For item b, channel c, sample
 * n, with every v_k zero before sample 0:
 *   T = clamp(decay_s, 0.01, 100),  g_k = 10^(-3 m_k / (sample_rate T)),  a = exp(-2 pi max(damping_hz, 0) / sample_rate)   (+inf: a = 0)
 *   r_k[n] = v_k[n - m_k],  u_k[n] = g_k r_k[n],  w_k[n] = x[n] + u_k[n] - (2/K) sum_j u_j[n],  v_k[n] = (1 - a) w_k[n] + a v_k[n - 1]
 *   wet[n] = K^(-1/2) sum_k s_ck r_k[n],  s_ck = (-1)^(k c) if decorrelate else 1,   y[n] = (1 - mix) x[n] + mix wet[n]
 * g_k and a are float64 in the kernels, rounded once to float32; everything after them is float32.
 * 1 <= K <= dasp_fdn_max_lines() = 16 and sum_k m_k <= dasp_fdn_max_delay_sum(K): the K rings of m_k + S floats and S staged words share
 * a workgroup's LDS. A row is walked in sequential steps of S = dasp_fdn_block(K, min_k m_k) = min(min_k m_k, 1024) samples.
 * Forward: v (NULL: not saved) receives the K line signals, which the backward pass reads.  Backward: gx (NULL: not written), gctl; r, w
 * and wet are recomputed from v; partials is scratch of dasp_fdn_partial_floats(B * C) = 18 floats per row, summed over an item's
 * channels in fp64 in a fixed order by a second launch. No atomics. y, v, gx and gctl are bit-identical run to run. The decay_s gradient
 * is zero where decay_s was clamped, the damping_hz gradient zero where damping_hz < 0 and at +inf. Backward with v = NULL writes gx
 * alone (it depends on no line signal), the same bits, in one launch: gctl and partials are not touched and may be NULL, gx may not.
 * dasp_fdn_prepare() raises the kernels' dynamic-LDS limit on the current device; the binding calls it once when it loads the library,
 * and the first call on a device that was not prepared does it itself.
 * A null pointer (v in forward and gx apart), a non-positive size, K outside 1 .. 16, an m_k < 1, a sample rate that is not positive and
 * finite: DASP_ERR_ARG (-1 from the queries); sum_k m_k above its maximum (K * shortest above it, for dasp_fdn_block) or B * C >= 2^31:
 * DASP_ERR_UNSUPPORTED (-2 from the queries). All of it is checked before any launch.
 * Non-finite input: a NaN or inf sample stays in the lines from then on. A NaN decay_s or damping_hz passes its clamp: the item's y, gx
 * and control gradients are NaN. No sample and no control forms an address. Other items keep every bit. */
int dasp_fdn_max_lines(void);
int dasp_fdn_block(int K, long shortest);
long dasp_fdn_max_delay_sum(int K);
long dasp_fdn_partial_floats(long rows);
int dasp_fdn_prepare(void);
int dasp_fdn_forward(const float* x, const float* ctl, const int* delays, float* y, float* v, int B, int C, long N, int K, double sample_rate,
                     int decorrelate, void* stream);
int dasp_fdn_backward(const float* x, const float* ctl, const int* delays, const float* v, const float* gy, float* gx, float* gctl,
                      float* partials, int B, int C, long N, int K, double sample_rate, int decorrelate, void* stream);

/* limiter: look-ahead brickwall limiter - hold, release and attack of the required gain reduction as a scan over the (max, x) semiring
 * and a box, one workgroup per ITEM, all channels linked (csrc/limiter.hip).
 * x, y, gy, gx (B, C, N) fp32; ctl, gctl (B, 2) fp32: threshold_db, release_ms; gain (B, N) fp32; winner (B, N) int32; lookahead = L in
 * samples, 0 <= L <= dasp_limiter_max_lookahead() = 1024.  For item b on the timeline m in [0, N + L), zero before 0, the level zero
 * from N on:
 *   thr = clamp(threshold_db, -120, 40),  t = clamp(release_ms, 0.1, 10000),  rho = exp(-ln 9 / (sample_rate t / 1000))
 *   p[m] = max_c |x[b,c,m]|  (lowest channel wins a tie),   r[m] = max(0, 20 log10(max(p[m], eps)) - thr)
 *   h[m] = max_{0<=k<=L} r[m-k]  (latest sample wins a tie),   e[m] = max(h[m], rho e[m-1])  (h wins a tie),   w[m] the winning sample of e[m]
 *   s[m] = (1/(L+1)) sum_{j=0..L} e[m-j],   G[m] = 10^(-s[m]/20),   y[b,c,n] = x[b,c,n] G[n+L]
 * so that |y| <= 10^(thr/20) at every sample, and an item below its threshold comes back bit for bit. r, the powers of rho, the box sum
 * and G are float64 in the kernels and rounded once; e is float32.
 * An item is walked in tiles of dasp_limiter_tile() = 2048 samples of the timeline.
 * Forward: gain and winner (both NULL: nothing saved) receive G[n+L] and w[n+L] (-1 where e = 0), n in [0, N):
 * dasp_limiter_state_floats(B, N) = 2 B N words, 8 bytes per sample of an item.  Backward: gx (NULL: not written), gctl; w[m] for m < L is
 * rebuilt from x; scratch: dasp_limiter_partial_floats(B, N) = 2 B N floats, the segmented sums of the winners' runs, zeroed by a kernel
 * of the call (it may be dirty). No atomics: y, gain, winner, gx and gctl are bit-identical run to run and for an item alone or in a batch.
 * Both control gradients are exactly zero where the control was clamped.
 * dasp_limiter_prepare() raises the kernels' dynamic-LDS limit on the current device; the binding calls it once when it loads the
 * library, and a call on a device that was not prepared does it itself.
 * A null pointer (gain and winner together in forward, gx in backward apart), a non-positive size, lookahead < 0, a sample rate that is not
 * positive and finite, an eps that is negative or not finite: DASP_ERR_ARG (-1 from the queries); lookahead above its maximum or
 * N >= 2^31 - 4096: DASP_ERR_UNSUPPORTED. All of it is checked before any launch.
 * Non-finite input: comparisons decide. A NaN peak asks for no reduction (the sample itself stays NaN), an inf peak for an infinite
 * one from there on. A NaN control makes y, gx and both control gradients of its item NaN. What the backward kernel reads from
 * winner is checked against [0, N) before it forms an address. Other items keep every bit. */
int dasp_limiter_tile(void);
int dasp_limiter_max_lookahead(void);
long dasp_limiter_state_floats(long B, long N);
long dasp_limiter_partial_floats(long B, long N);
int dasp_limiter_prepare(void);
int dasp_limiter_forward(const float* x, const float* ctl, float* y, float* gain, int* winner, int B, int C, long N, int lookahead,
                         double sample_rate, double eps, void* stream);
int dasp_limiter_backward(const float* x, const float* ctl, const float* gain, const int* winner, const float* gy, float* gx, float* gctl,
                          float* scratch, int B, int C, long N, int lookahead, double sample_rate, double eps, void* stream);

/* phaser:`stages` first-order all-pass sections in series whose shared coefficient a sine LFO sweeps, mixed with the dry signal; a
 * recurrence whose coefficient changes with every sample, evaluated as a scan, one workgroup per (b, c) row (csrc/phaser.hip).
 * x, y, gy, gx (B, C, N) fp32; ctl, gctl (B, 5) fp32: rate_hz, center_hz, depth (octaves), phase (turns), mix.  For item b, channel c,
 * sample n, with every state zero before sample 0:
 *   theta = 2 pi (rate_hz n / sample_rate + phase + c stereo_spread)
 *   f = clamp(center_hz 2^(depth sin theta), sample_rate/4096, 0.49 sample_rate),  t = tan(pi f / sample_rate),  a = (t - 1) / (t + 1)
 *   s_0 = x,  s_k[n] = a[n] (s_{k-1}[n] - s_k[n-1]) + s_{k-1}[n-1]  (k = 1 .. stages),   y[n] = (1 - mix) x[n] + mix s_stages[n]
 * The phase is float64 in the kernels and reduced to a turn before it is rounded; everything after it is float32.
 * A row is walked in tiles of dasp_phaser_tile(stages) samples, 1 <= stages <= dasp_phaser_max_stages().
 * Forward: states (NULL: not saved) receives dasp_phaser_state_floats(B * C, N, stages) = rows * ceil(N / tile) * stages floats, the
 * stage states before every tile - all the backward pass needs beyond x and ctl.  Backward: gx (NULL: not written), gctl; the stage
 * signals of a tile are rebuilt from states; partials is scratch of dasp_phaser_partial_floats(B * C) = 5 floats per row, summed over
 * an item's channels in fp64 in a fixed order by a second launch. No atomics. y, states, gx and gctl are bit-identical run to run.
 * The gradients of rate_hz, center_hz, depth and phase take no contribution from samples where f was clamped.
 * dasp_phaser_prepare() raises the backward kernel's dynamic-LDS limit on the current device; the binding calls it once when it loads
 * the library, and the first backward call on a device that was not prepared does it itself.
 * A null pointer (states in forward and gx apart), a non-positive size, stages < 1, a sample rate that is not positive and finite or a
 * non-finite stereo_spread: DASP_ERR_ARG (-1 from the queries); stages above its maximum or B * C >= 2^31: DASP_ERR_UNSUPPORTED (-2
 * from the queries). All of it is checked before any launch.
 * Non-finite input: a NaN or inf sample stays in the stages' states - it reaches every later sample of its row. A NaN control passes
 * the clamp and makes the item's y, gx and control gradients NaN (a NaN mix its own gradient too, which holds no term with mix). Other
 * items keep every bit. */
int dasp_phaser_max_stages(void);
int dasp_phaser_tile(int stages);
long dasp_phaser_state_floats(long rows, long N, int stages);
long dasp_phaser_partial_floats(long rows);
int dasp_phaser_prepare(void);
int dasp_phaser_forward(const float* x, const float* ctl, float* y, float* states, int B, int C, long N, int stages, double sample_rate,
                        double stereo_spread, void* stream);
int dasp_phaser_backward(const float* x, const float* ctl, const float* states, const float* gy, float* gx, float* gctl, float* partials, int B,
                         int C, long N, int stages, double sample_rate, double stereo_spread, void* stream);

/* time_varying_filter: Simper's trapezoidal state-variable filter (the published Cytomic form) whose cutoff and resonance follow control
 * curves; a recurrence that couples two states, evaluated as a scan over 2 x 2 affine maps, one workgroup per (b, c) row
 * (csrc/tvfilter.hip). x, y, gy, gx (B, C, N) fp32; cutoff_hz, q, gcutoff, gq (B, F) fp32, F = dasp_tvfilter_frames(N, hop) =
 * ceil(N / hop) + 1, shared by an item's channels; mix, gmix (B) fp32. hop: a power of two from 8 to 2048. mode: 0 lowpass, 1 bandpass,
 * 2 highpass, 3 notch. For item b, every channel and sample n, with both states zero before sample 0:
 *   G_j = tan(pi clamp(cutoff_hz[b,j], sample_rate/4096, 0.49 sample_rate) / sample_rate),  K_j = 1 / clamp(q[b,j], 0.1, 100)
 *                                                                                        (float64, then rounded once to float32)
 *   j = n / hop,  t = (n mod hop) / hop,  g = G_j + t (G_{j+1} - G_j),  k = K_j + t (K_{j+1} - K_j)          (float32 from here on)
 *   a1 = 1 / (1 + g (g + k)),  a2 = g a1,  a3 = g a2
 *   v3 = x[n] - ic2,  v1 = a1 ic1 + a2 v3,  v2 = ic2 + a2 ic1 + a3 v3,  ic1 <- 2 v1 - ic1,  ic2 <- 2 v2 - ic2
 *   w = v2 | k v1 | x - k v1 - v2 | x - k v1  by mode,   y[n] = (1 - mix) x[n] + mix w
 * A row is walked in tiles of dasp_tvfilter_tile() samples.
 * Forward: states (NULL: not saved) receives dasp_tvfilter_state_floats(B * C, N) = rows * ceil(N / tile) * 2 floats, (ic1, ic2) before
 * every tile - all the backward pass needs beyond x and the curves.  Backward: gx (NULL: not written), gcutoff, gq, gmix; scratch holds
 * dasp_tvfilter_scratch_floats(B * C, N, hop) = rows * (2 F + 1) floats, the rows' sums per frame point, added over an item's channels
 * in fp64 in a fixed order by a second launch. No atomics. y, states, gx, gcutoff, gq and gmix are bit-identical run to run.
 * gcutoff and gq are exactly zero where the frame value was clamped.
 * A null pointer (states in forward and gx apart), a non-positive size or hop, a mode outside 0 .. 3 or a sample rate that is not positive
 * and finite: DASP_ERR_ARG (-1 from the queries); a hop that is no power of two from 8 to 2048, B * C >= 2^31 or B * F >= 2^37:
 * DASP_ERR_UNSUPPORTED (-2 from the queries). All of it is checked before any launch.
 * Non-finite input: a NaN or inf sample stays in the states - it reaches every later sample of its row. The clamps are comparisons,
 * which a NaN passes: a NaN frame value j makes its item NaN from sample (j - 1) hop on; earlier samples and other items keep every bit. */
int dasp_tvfilter_tile(void);
long dasp_tvfilter_frames(long N, int hop);
long dasp_tvfilter_state_floats(long rows, long N);
long dasp_tvfilter_scratch_floats(long rows, long N, int hop);
int dasp_tvfilter_forward(const float* x, const float* cutoff_hz, const float* q, const float* mix, float* y, float* states, int B, int C, long N,
                          int hop, int mode, double sample_rate, void* stream);
int dasp_tvfilter_backward(const float* x, const float* cutoff_hz, const float* q, const float* mix, const float* states, const float* gy, float* gx,
                           float* gcutoff, float* gq, float* gmix, float* scratch, int B, int C, long N, int hop, int mode, double sample_rate,
                           void* stream);

/* time_varying_eq: a bell, low-shelf or high-shelf band of the same trapezoidal state-variable filter whose gain, cutoff and Q follow
 * control curves (csrc/tveq.hip, on the walk of csrc/tvfilter.hip). x, y, gy, gx (B, C, N) fp32; gain_db, cutoff_hz, q, ggain, gcutoff,
 * gq (B, F) fp32, F = dasp_tvfilter_frames(N, hop) = ceil(N / hop) + 1, shared by an item's channels. hop: a power of two from 8 to
 * 2048. mode: 0 bell, 1 lowshelf, 2 highshelf. For item b, every channel and sample n, with both states zero before sample 0:
 *   A_j = 10^(clamp(gain_db[b,j], -40, 40) / 40),  T_j = tan(pi clamp(cutoff_hz[b,j], sample_rate/4096, 0.49 sample_rate) / sample_rate),
 *   Qc = clamp(q[b,j], 0.1, 100)                                                        (float64, then G, K, A rounded once to float32)
 *   bell: G_j = T_j, K_j = 1 / (Qc A_j)    lowshelf: G_j = T_j / sqrt A_j, K_j = 1 / Qc    highshelf: G_j = T_j sqrt A_j, K_j = 1 / Qc
 *   j = n / hop,  t = (n mod hop) / hop,  g = G_j + t (G_{j+1} - G_j),  likewise k from K and A from A_j        (float32 from here on)
 *   a1, a2, a3, v1, v2, ic1, ic2 as for time_varying_filter
 *   y[n] = x + k (A^2 - 1) v1  |  x + k (A - 1) v1 + (A^2 - 1) v2  |  A^2 x + k (1 - A) A v1 + (1 - A^2) v2   by mode
 * An all-zero gain_db gives y = x and gx = gy bit for bit. A row is walked in tiles of dasp_tveq_tile() samples.
 * Forward: states (NULL: not saved) receives dasp_tveq_state_floats(B * C, N) = rows * ceil(N / tile) * 2 floats, (ic1, ic2) before
 * every tile - all the backward pass needs beyond x and the curves.  Backward: gx (NULL: not written), ggain, gcutoff, gq; scratch holds
 * dasp_tveq_scratch_floats(B * C, N, hop) = rows * 3 F floats, the rows' sums per frame point for G, K and A, added over an item's
 * channels and chained to the three curves in fp64 in a fixed order by a second launch. No atomics. y, states, gx, ggain, gcutoff and gq
 * are bit-identical run to run. Each gradient is exactly zero where its frame value was clamped.
 * A null pointer (states in forward and gx apart), a non-positive size or hop, a mode outside 0 .. 2 or a sample rate that is not positive
 * and finite: DASP_ERR_ARG (-1 from the queries); a hop that is no power of two from 8 to 2048, B * C >= 2^31 or B * F >= 2^37:
 * DASP_ERR_UNSUPPORTED (-2 from the queries). All of it is checked before any launch.
 * Non-finite input: as for time_varying_filter, for all three curves - a NaN frame value j makes its item NaN from sample (j - 1) hop on;
 * earlier samples and other items keep every bit. */
int dasp_tveq_tile(void);
long dasp_tveq_state_floats(long rows, long N);
long dasp_tveq_scratch_floats(long rows, long N, int hop);
int dasp_tveq_forward(const float* x, const float* gain_db, const float* cutoff_hz, const float* q, float* y, float* states, int B, int C, long N,
                      int hop, int mode, double sample_rate, void* stream);
int dasp_tveq_backward(const float* x, const float* gain_db, const float* cutoff_hz, const float* q, const float* states, const float* gy, float* gx,
                       float* ggain, float* gcutoff, float* gq, float* scratch, int B, int C, long N, int hop, int mode, double sample_rate,
                       void* stream);

/* envelope_follower and gain_curve: the control-rate side chains, audio -> curve and curve -> gain (csrc/envelope.hip). x, gx, y, gy
 * (B, C, N) fp32; smoothing_ms, gsmoothing (B) fp32; env, tangent, genv, gain_db, ggain (B, F) fp32, F = ceil(N / hop) + 1 (the frame
 * points of dasp_tvfilter_frames: point j at sample j hop), shared by an item's channels. hop: a power of two from 8 to 2048.
 * detector: 0 peak, 1 power. Both ops work in tiles of dasp_envelope_tile() samples, one workgroup per (item, tile).
 * envelope, for item b with the level zero from sample N on and e[-1] = 0:
 *   t = clamp(smoothing_ms, 0.1, 10000),  a = exp(-ln 9 / (sample_rate t / 1000))
 *   p[m] = max_c |x[b,c,m]|  (the lowest channel wins a tie)  |  mean_c x[b,c,m]^2
 *   e[m] = a e[m-1] + (1 - a) p[m],   env[b,j] = e[j hop]
 * evaluated as per-block sums z_j = sum_{i=1..hop} (1 - a) a^(hop-i) p[(j-1) hop + i] in fp32 with weights from fp64 and the frame-rate
 * recurrence E_j = a^hop E_{j-1} + z_j in fp64. tangent (NULL: not formed) receives dE_j/da, which is all the backward pass needs beyond
 * x and the control. scratch: dasp_envelope_scratch_floats(B, N, hop) = 2 B F floats, in both directions (backward: NULL when gx is).
 * Backward: gx (NULL: not written) and gsmoothing (NULL exactly when tangent is; exactly zero where the control was clamped).
 * gain_curve: j = n / hop, t = (n mod hop) / hop, g = gain_db[b,j] + t (gain_db[b,j+1] - gain_db[b,j]) (the frame value itself at
 * t = 0), y[b,c,n] = x[b,c,n] 10^(g / 20). Backward: gx (NULL: not written) and ggain (NULL: not formed; else scratch holds
 * dasp_gaincurve_scratch_floats(B, N, hop) = 2 B F floats, the per-interval pairs that a second launch joins).
 * No atomics: every output is bit-identical run to run and for an item alone or in a batch.
 * A null pointer (the optional ones apart), a non-positive size or hop, a detector outside 0 .. 1 or a sample rate that is not positive
 * and finite: DASP_ERR_ARG (-1 from the queries); a hop that is no power of two from 8 to 2048, N > 2^40, B * tiles >= 2^31 or
 * B * F >= 2^37: DASP_ERR_UNSUPPORTED (-2 from the queries). All of it is checked before any launch.
 * Non-finite input: a NaN smoothing_ms makes env, tangent and the gradients of its item NaN; a NaN or inf sample m0 reaches the frame
 * points j hop >= m0 of its item; a NaN gain_db[b,j] reaches the samples (j - 1) hop < n < (j + 1) hop of its item. */
int dasp_envelope_tile(void);
long dasp_envelope_scratch_floats(long B, long N, int hop);
int dasp_envelope_forward(const float* x, const float* smoothing_ms, float* env, float* tangent, float* scratch, int B, int C, long N, int hop,
                          int detector, double sample_rate, void* stream);
int dasp_envelope_backward(const float* x, const float* smoothing_ms, const float* tangent, const float* genv, float* gx, float* gsmoothing,
                           float* scratch, int B, int C, long N, int hop, int detector, double sample_rate, void* stream);
long dasp_gaincurve_scratch_floats(long B, long N, int hop);
int dasp_gaincurve_forward(const float* x, const float* gain_db, float* y, int B, int C, long N, int hop, void* stream);
int dasp_gaincurve_backward(const float* x, const float* gain_db, const float* gy, float* gx, float* ggain, float* scratch, int B, int C, long N,
                            int hop, void* stream);

/* block_level and ballistics: the detector and the attack / release smoother of the control-rate layer, audio -> curve and
 * curve -> curve (csrc/ballistics.hip). The frame points are those of the envelope: F = ceil(N / hop) + 1, point j at sample j hop,
 * hop a power of two from 8 to 2048. x, gx (B, C, N) fp32; level, glevel (B, F) fp32; winners (B, F) int32; detector: 0 peak, 1 power.
 * block_level, with p[m] the level of dasp_envelope_forward (p = 0 from sample N on):
 *   level[b,0] = p[0],   level[b,j] = max_{i=1..hop} p[(j-1) hop + i]  (peak)  |  (1 / hop) sum_{i=1..hop} p[(j-1) hop + i]  (power)
 * one workgroup per (item, tile of dasp_envelope_tile() samples). Peak: the earliest sample of a block that holds the maximum wins, on
 * its lowest winning channel, and the first NaN sample of a block wins it; winners (NULL: not written; unused by power) receives per
 * frame (i - 1) | sign << 11 | channel << 13 for the winning sample (j-1) hop + i, sign 0 zero, 1 positive, 2 negative, 3 NaN.
 * Backward: peak reads winners and glevel alone (x may be NULL) and writes gx = sign(x_winner) glevel[b,j] at the winner and zero
 * everywhere else; power reads x (winners may be NULL), gx = 2 x / (C hop) glevel[b,j], and 2 x / C glevel[b,0] for sample 0.
 * ballistics, for item b over any F >= 1 values of a curve, E_{-1} = 0:
 *   t_a = clamp(attack_ms, 0.1, 10000),  c_a = -expm1(-ln 9 hop / (sample_rate t_a / 1000)),  c_r likewise from release_ms
 *   up[b,j] = curve[b,j] > E_{j-1},   c_j = up ? c_a : c_r,   out[b,j] = E_j = E_{j-1} + c_j (curve[b,j] - E_{j-1})
 * walked in fp64 by one wave per item over chunks of dasp_ballistics_chunk() frames staged through LDS, rounded once to fp32.
 * curve, out, gout, gcurve (B, F) fp32; up (B, F) bytes (forward: NULL, not written); attack_ms, release_ms, gattack, grelease (B) fp32.
 * Backward takes the forward's out and up: Lambda_j = gout_j + (1 - c_{j+1}) Lambda_{j+1}, gcurve_j = c_j Lambda_j, gattack =
 * (dc_a/dt_a) sum over the frames with up of Lambda_j (curve_j - out_{j-1}), grelease over the others; each of the three outputs may be
 * NULL (not all); a control gradient is exactly zero where its control was clamped.
 * No atomics: every output is bit-identical run to run and for an item alone or in a batch.
 * A null pointer (the optional ones apart), a non-positive size or hop, a detector outside 0 .. 1 or a sample rate that is not positive
 * and finite: DASP_ERR_ARG; a hop that is no power of two from 8 to 2048, more than 2^18 channels, N > 2^40, B * tiles >= 2^31 or
 * B * F >= 2^37: DASP_ERR_UNSUPPORTED. All of it is checked before any launch.
 * Non-finite input: a NaN sample m0 reaches frame ceil(m0 / hop) of level; a NaN curve value j makes out NaN from j on in its item; a
 * NaN attack_ms or release_ms makes out and every gradient of its item NaN. */
int dasp_ballistics_chunk(void);
int dasp_blocklevel_forward(const float* x, float* level, int* winners, int B, int C, long N, int hop, int detector, void* stream);
int dasp_blocklevel_backward(const float* x, const int* winners, const float* glevel, float* gx, int B, int C, long N, int hop, int detector,
                             void* stream);
int dasp_ballistics_forward(const float* curve, const float* attack_ms, const float* release_ms, float* out, unsigned char* up, int B, long F,
                            int hop, double sample_rate, void* stream);
int dasp_ballistics_backward(const float* curve, const float* attack_ms, const float* release_ms, const float* out, const unsigned char* up,
                             const float* gout, float* gcurve, float* gattack, float* grelease, int B, long F, int hop, double sample_rate,
                             void* stream);

/* resample: polyphase windowed-sinc sample-rate conversion by the reduced ratio orig : new_ = o : n, and its adjoint
 * (csrc/resample.hip; the definition is DESIGN.md 3.15, a restatement of torchaudio.functional.resample's published algorithm with
 * the taps exactly zero where the window's argument was clamped). x, gx (rows, N) fp32; y, gy (rows, M) fp32, M = ceil(n N / o):
 *   forward   y[q n + r] = sum_k h[r][k] x[q o + k - width]        x zero outside [0, N)
 *   backward  gx[i] = sum over the (q, r) whose span covers i of h[r][i + width - q o] gy[q n + r]       a gather, no atomics
 * Both directions are one form, out[Q A + p] = sum_{m < cnt[p]} T[m][p] in[Q B + off[p] + m], forward with (A, B) = (n, o), backward
 * with (A, B) = (o, n); `table` is that direction's table in device memory, dasp_resample_table_words(A, taps) = A taps + A 32-bit
 * words: the float32 taps tap-major, T[m A + p], zero for m >= cnt[p], then per phase (off[p] - lo) | cnt[p] << 16, with
 * taps = max cnt, lo = min off, span = max (off + cnt) - lo. The host builds both in float64 and rounds once
 * (dasp_pytorch_amd/_resample_design.py); dasp_resample_table_store copies host words into device memory with kernels that carry them
 * in their arguments - kernel nodes under stream capture, no copy from host memory.
 * One workgroup computes dasp_resample_tile(A, B, taps, span) consecutive outputs of one row: a whole number of frames of A outputs,
 * about 2048 where the staged input window (at most dasp_resample_window_limit() = 20480 words) allows it. A table of more than
 * dasp_resample_table_limit() = 16384 taps, a span beyond the window limit, or table and window together beyond 158 KiB of LDS:
 * DASP_ERR_UNSUPPORTED (-2 from the queries), as are more than 2^31 - 1 workgroups. A null pointer, a non-positive size, taps < 1,
 * span < taps, M other than ceil(n N / o), lo outside [-20480, B]: DASP_ERR_ARG (-1 from the queries). All of it is checked before any
 * launch. dasp_resample_prepare() raises the kernels' dynamic-LDS limit on the current device; the binding calls it once when it
 * loads the library, and the first call on a device that was not prepared does it itself.
 * Exactly cnt[p] products are formed per output, in ascending m, float32 FMAs from zero: an output depends on its phase and its
 * inputs only - y and gx are bit-identical run to run, for a row alone or in a batch. A NaN or inf sample reaches exactly the outputs
 * whose span covers it (in the conv1d form of the same filter it reaches every output of the 2 width + o window). */
int dasp_resample_table_limit(void);
int dasp_resample_window_limit(void);
int dasp_resample_tile(int out_period, int in_period, int taps, int span);
long dasp_resample_table_words(int out_period, int taps);
int dasp_resample_prepare(void);
int dasp_resample_table_store(void* dst, const void* host_words, long words, void* stream);
int dasp_resample_forward(const float* x, const void* table, float* y, long rows, long N, long M, int orig, int new_, int taps, int lo, int span,
                          void* stream);
int dasp_resample_backward(const float* gy, const void* table, float* gx, long rows, long N, long M, int orig, int new_, int taps, int lo, int span,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-resolution STFT loss, the op downstream of the effect chain in the reference's training loops
 * (auraloss.freq.MultiResolutionSTFTLoss(): examples/style_transfer.py:341,363, auto_eq.py:252, virtual_analog.py:288; auraloss is
 * not vendored by the reference - its published algorithm is restated in oracle/dasp_oracle.py:mrstft_loss).
 * pred, target: (rows, N) fp32.  Resolutions: nres <= 8 triples (fft, hop, win); fft a power of two in 8..8192 (8192: one frame per
 * 1024-thread workgroup), win <= fft, fft/2 < N.  tw: 4096 complex twiddles from dasp_mrstft_table.
 * Per resolution w_sc * SC + w_log_mag * LOG + w_lin_mag * LIN (auraloss's term weights; LIN = mean ||X| - |Y||), mean over the
 * resolutions; a weight of exactly 0 leaves its term out of the loss and the gradient; (1, 1, 0) are auraloss's defaults.
 * n_bins = 0 and mel_tables = NULL: linear bins. n_bins > 0: the terms on mel-scaled magnitudes (below), 1 <= n_bins <= min(256,
 * fft / 2 + 1) for every resolution, mel_tables a host array of nres non-null device pointers, table r for fft[r]. One without the other,
 * a null pointer elsewhere or a wrt_target other than 0 or 1: DASP_ERR_ARG before any launch; resolutions, n_bins or weights that are not
 * supported (and rows > 65535): DASP_ERR_UNSUPPORTED, and -1 from the size query.
 * partials: dasp_mrstft_partial_floats floats.  stats: 4*nres floats (forward -> backward).  loss, gloss: device scalars, the loss
 * bit-identical run to run (fixed summation order).  grad (rows, N) is overwritten with gloss * d loss / d pred, or with wrt_target = 1
 * gloss * d loss / d target (auraloss differentiates both arguments; the same kernels with the signals swapped), through float atomics:
 * summation order only is not deterministic.
 * Non-finite samples: the clamp of the bin powers is torch.clamp(min = eps), not fmax - a NaN or +-inf sample makes every bin of the
 * frames that hold it non-finite, so the loss (and stats) of that call are NaN / inf, as auraloss's are; it is never read as silence.
 * Gradient: with w_sc != 0 every row is non-finite (all rows share the norms of the spectral convergence); with w_sc = 0 the rows of
 * the other signals keep the values of a batch without the bad sample (up to the order of the atomics) and the row that holds the
 * sample is non-finite over those frames. The buffers of a later call are not affected (grad is zeroed by every backward call). The
 * sum / difference loss likewise, per item.
 * ------------------------------------------------------------------------------------------- */
long dasp_mrstft_partial_floats(long rows, int N, int nres, const int* fft, const int* hop, const int* win, int n_bins);
int dasp_mrstft_table(void* tw, void* stream);
int dasp_mrstft_forward(const float* pred, const float* target, const void* tw, const void* const* mel_tables, float* partials,
                        float* stats, float* loss, int rows, int N, int nres, const int* fft, const int* hop, const int* win, float eps,
                        float w_sc, float w_log_mag, float w_lin_mag, int n_bins, void* stream);
int dasp_mrstft_backward(const float* pred, const float* target, const void* tw, const void* const* mel_tables, const float* stats,
                         const float* gloss, float* grad, int rows, int N, int nres, const int* fft, const int* hop, const int* win,
                         float eps, float w_sc, float w_log_mag, float w_lin_mag, int n_bins, int wrt_target, void* stream);
/* The perceptual weighting of the loss (auraloss FIRFilter(filter_type="aw", ntaps=101), applied to both signals before the STFTs):
 * y[n] = sum_k taps[k] x[n + k - ntaps/2] over rows of N samples, zeros outside [0, N) (conv1d(x, taps, padding=ntaps/2)); ntaps odd,
 * <= 101; taps on the device. Fixed summation order: bit-identical run to run. dasp_fir_same_forward filters x0 -> y0 and x1 -> y1;
 * dasp_fir_same_adjoint is its adjoint (the taps reversed) on g0 -> gx0 and g1 -> gx1. The second pair may be NULL (one signal).
 * dasp_fir_taps_store writes ntaps host floats to dst through a kernel's arguments (no host-memory copy: capturable into a graph). */
int dasp_fir_same_forward(const float* x0, const float* x1, float* y0, float* y1, const float* taps, int ntaps, int rows, int N,
                          void* stream);
int dasp_fir_same_adjoint(const float* g0, const float* g1, float* gx0, float* gx1, const float* taps, int ntaps, int rows, int N,
                          void* stream);
int dasp_fir_taps_store(float* dst, const float* host_taps, int ntaps, void* stream);
/* Mel-scaled magnitudes (auraloss scale="mel", n_bins; auraloss.freq.MelSTFTLoss): per frame M = W |X| with
 * W = librosa.filters.mel(sr, n_fft, n_mels) (n_bins x (n_fft / 2 + 1), Slaney scale and normalisation, not clamped after the projection),
 * the sums and the mean over rows x frames x n_bins.
 * One device table per resolution (dasp_mel_table_floats floats; -1: n_fft not a power of two in 8..8192 or n_bins outside 1..min(256,
 * n_fft / 2 + 1)): per bin the first filter it lies in and its weights in that filter and
 * the next, per filter its first bin and bin count. dasp_mel_table_store builds it on the device in fp64 from the n_bins + 2 edge
 * frequencies in Hz (host fp64, increasing, passed on as kernel arguments: capturable into a graph); dasp_mel_table_dense writes the
 * (n_bins, n_fft / 2 + 1) float matrix a table stands for. */
long dasp_mel_table_floats(int n_fft, int n_bins);
int dasp_mel_table_store(float* table, const double* host_edges, double sample_rate, int n_fft, int n_bins, void* stream);
int dasp_mel_table_dense(const float* table, float* dense, int n_fft, int n_bins, void* stream);
/* The sum / difference loss of a stereo pair (auraloss.freq.SumAndDifferenceSTFTLoss): the loss above on L + R and on L - R as two
 * separate losses, each with its own sums and its own means over the `items` rows of its half, from one launch per resolution and direction (a workgroup owns both channels of an item).
 * pred, target: (items, 2, N) fp32, channel rows interleaved (row 2 b = left, 2 b + 1 = right of item b). Resolutions, weights, n_bins,
 * mel_tables, wrt_target and the refusals as for dasp_mrstft_* (every size runs the generic-geometry kernels, one workgroup per
 * frame group of an item). partials: dasp_mrstft_sd_partial_floats floats (2 x nres x items x groups x 4; -1: not supported).
 * stats: 8 * nres floats, [(half * nres + res) * 4 + c], half 0 = sum, 1 = difference (forward -> backward). loss: 2 floats, (sum_loss,
 * diff_loss), bit-identical run to run. gloss: 2 device floats, d objective / d sum_loss and d objective / d diff_loss; grad
 * (items, 2, N) is overwritten with gloss[0] d sum_loss / d x + gloss[1] d diff_loss / d x, x = pred or target: both halves' gradient
 * spectra go back to channels in the frequency domain and through one packed inverse transform, one float atomic per sample, frame and
 * channel. */
long dasp_mrstft_sd_partial_floats(long items, int N, int nres, const int* fft, const int* hop, const int* win, int n_bins);
int dasp_mrstft_sd_forward(const float* pred, const float* target, const void* tw, const void* const* mel_tables, float* partials,
                           float* stats, float* loss, int items, int N, int nres, const int* fft, const int* hop, const int* win,
                           float eps, float w_sc, float w_log_mag, float w_lin_mag, int n_bins, void* stream);
int dasp_mrstft_sd_backward(const float* pred, const float* target, const void* tw, const void* const* mel_tables, const float* stats,
                            const float* gloss, float* grad, int items, int N, int nres, const int* fft, const int* hop, const int* win,
                            float eps, float w_sc, float w_log_mag, float w_lin_mag, int n_bins, int wrt_target, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Time-domain losses.  Replaces auraloss.time.ESRLoss, DCLoss, LogCoshLoss, SNRLoss, SISDRLoss and SDSDRLoss (auraloss 0.4.0; not
 * vendored by the reference - restated in tests/auraloss_time_restated.py) and the MSE term of the reference's
 * examples/virtual_analog.py:299,324-326, as ONE weighted sum from one pass (csrc/tdloss.hip). Per row of N samples, d = p - t:
 *   esr      sum d^2 / (sum t^2 + eps)                      dc    mean(d)^2 / (mean(t^2) + eps)
 *   log_cosh mean(log(cosh(a d) + eps)) / a                 mse   mean(d^2)
 *   snr      -10 log10(sum t^2 / (sum d^2 + eps) + eps)
 *   si_sdr   alpha = sum p t / (sum t^2 + eps);  -10 log10(sum (alpha t)^2 / (sum (p - alpha t)^2 + eps) + eps)
 *   sd_sdr   same alpha;                         -10 log10(sum (alpha t)^2 / (sum d^2 + eps) + eps)
 * zero_mean != 0: snr, si_sdr and sd_sdr are taken on the signals minus their row means. A weight of exactly 0 leaves its term out of the
 * value and the gradient (no 0 * inf); the weights, a > 0 and eps must be finite and one weight non-zero (DASP_ERR_ARG otherwise).
 * reduction: 0 = none, 1 = mean over the rows, 2 = sum over the rows (of the per-row values: the mse term stays a per-row mean).
 *   pred, target  (rows, N) fp32, contiguous; any 4-byte aligned address
 *   scratch       dasp_tdloss_scratch_doubles(rows, N) doubles (-1: sizes not supported), written and read by the forward call only
 *   moments       6 * rows doubles, [row][sum d, sum t, sum d^2, sum t^2, sum d t, sum log(cosh(a d) + eps)] (forward -> backward; the
 *                 last one is 0 when w_log_cosh = 0)
 *   row_loss      rows floats, the weighted loss of every row;  loss: 1 float, their mean / sum (not written, may be NULL, for reduction 0)
 *   gloss         the upstream gradient on the device: 1 float for reduction 1 / 2, rows floats for reduction 0
 *   gpred, gtarget  (rows, N) fp32, overwritten with gloss * d loss / d pred and d loss / d target in one launch; either may be NULL
 * The backward call takes the options of the forward call that wrote `moments`. No atomics and nothing zeroed: loss and gradients are
 * bit-identical run to run, and both calls are plain kernel launches on `stream` (capturable into a graph).
 * Non-finite samples: a NaN or +-inf sample makes the moments of ITS row non-finite and the row's loss what auraloss's formula gives
 * on them - NaN or inf for every term (zero_mean included: the centred sums are clamped at 0 with `x < 0 ? 0 : x`, which hands a NaN
 * on, so a diverged prediction never reads as a perfect SNR), the one finite case being snr of a +inf prediction with zero_mean = 0,
 * -10 log10(eps) = 80 dB at eps = 1e-8. Every other row keeps its loss and its gradients bit for bit; reduction 1 / 2 are non-finite
 * when a row is.
 * ------------------------------------------------------------------------------------------- */
long dasp_tdloss_scratch_doubles(long rows, long N);
int dasp_tdloss_forward(const float* pred, const float* target, double* scratch, double* moments, float* row_loss, float* loss, long rows,
                        long N, double w_esr, double w_dc, double w_log_cosh, double w_snr, double w_si_sdr, double w_sd_sdr, double w_mse,
                        double a, double eps, int zero_mean, int reduction, void* stream);
int dasp_tdloss_backward(const float* pred, const float* target, const double* moments, const float* gloss, float* gpred, float* gtarget,
                         long rows, long N, double w_esr, double w_dc, double w_log_cosh, double w_snr, double w_si_sdr, double w_sd_sdr,
                         double w_mse, double a, double eps, int zero_mean, int reduction, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Filters longer than one biquad.  Replaces dasp_pytorch.signal.lfilter_via_fsm (dasp_pytorch/signal.py:95-133) for K = 4 .. 16
 * coefficients per row (orders 3 .. 15; K <= 3 goes through the cascaded-biquad entry points above; the reference's only caller uses
 * K = 2, functional.py:372-380). Exact recurrence in double arithmetic, one thread per (row, chunk of time); the chunks run side by side
 * and are stitched by their state transition (csrc/lfilter.hip: three launches per direction).
 *   x, y, gy, gx: (rows, N) float (f64 = 0) or double (f64 = 1);  bn, an: (Bs, K) doubles, Bs = rows or 1, normalised so that
 *   an[:, 0] = 1 (FIR: an = 1, 0, ...);  wsave: (N, rows) doubles written by the forward pass for the backward pass (NULL: none follows);
 *   work: dasp_lfilter_work_doubles(rows, N, K, chunk) doubles of scratch, its size passed as work_doubles (checked: DASP_ERR_ARG);
 *   chunk: samples per chunk of time, 0 = the library's plan (1024 from 16 chunks on). The size query, the forward and the backward call of
 *   one filter operation must be given the same value; the library reads no environment variable for it (round 4, advisor finding);
 *   gb, ga: (rows, K) doubles, per row (the caller adds the rows of a broadcast filter; ga[:, 0] = 0);  gx may be NULL.
 * ------------------------------------------------------------------------------------------- */
long dasp_lfilter_work_doubles(int rows, long N, int K, long chunk);
int dasp_lfilter_forward(const void* x, const double* bn, const double* an, int Bs, void* y, double* wsave, double* work, long work_doubles,
                         int rows, long N, int K, int f64, long chunk, void* stream);
int dasp_lfilter_backward(const void* gy, const double* bn, const double* an, int Bs, const double* wsave, void* gx, double* gb,
                          double* ga, double* work, long work_doubles, int rows, long N, int K, int f64, long chunk, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frequency responses.  Replaces dasp_pytorch.signal.fft_freqz (dasp_pytorch/signal.py:7-11) and fft_sosfreqz (:14-32): the response of
 * a cascade of S rational sections on the rFFT grid, H_k = prod_s B_s(z_k) / A_s(z_k), z_k = e^{-2 pi i k / n}, k = 0 .. n/2, evaluated
 * per bin in fp64 (csrc/freqz.hip) instead of two zero-padded FFTs per section. a0 is not normalised; taps j >= n_fft are cropped, as
 * torch.fft.rfft crops its input.
 *   b: (rows, S, Kb), a: (rows, S, Ka) contiguous, float (f64 = 0) or double (f64 = 1);  H, gH: (rows, n_fft/2 + 1) interleaved complex
 *   of the same precision;  gb, ga: like b, a (gradient sum_k Re(conj(dH_k/dc) gH_k));  1 <= S <= 16, 1 <= Kb, Ka <= 32 and at most 96
 *   terms S (min(Kb, n) + min(Ka, n)), else DASP_ERR_UNSUPPORTED;  work: dasp_freqz_work_doubles(...) doubles of scratch, its size passed
 *   as work_doubles (checked: DASP_ERR_ARG). The backward call is two launches (partials per workgroup, then a finalize that sums them in
 *   a fixed order): no float atomics, bit-identical results run to run.
 * ------------------------------------------------------------------------------------------- */
long dasp_freqz_work_doubles(int rows, int S, int Kb, int Ka, long n_fft);
int dasp_freqz_forward(const void* b, const void* a, int rows, int S, int Kb, int Ka, long n_fft, int f64, void* H, void* stream);
int dasp_freqz_backward(const void* b, const void* a, const void* gH, int rows, int S, int Kb, int Ka, long n_fft, int f64, double* work,
                        long work_doubles, void* gb, void* ga, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Filtering by a supplied frequency response.  Replaces dasp_pytorch.signal.freqdomain_fir (dasp_pytorch/signal.py:35-39):
 * y = irfft(rfft(x, n_fft) * H, n_fft), circular convolution, not cropped (csrc/fdfir.hip).
 *   x, gx: (rows, T) fp32, T >= 1 (zero-padded to n_fft, or cropped to it; gx is 0 for cropped samples);  y, gy: (rows, n_fft) fp32;
 *   H, gH: (h_rows, n_fft/2 + 1) interleaved complex fp32 in natural rfft order, rows = h_rows * chs: the chs consecutive rows of an item
 *   share one response (h_rows = rows: a response per row). The imaginary parts of bins 0 and n_fft/2 are ignored; their gradient is 0.
 *   gH = w_k / n conj(X_k) GY_k summed over the item's rows in a fixed order (no atomics; PyTorch's complex-gradient convention).
 *   n_fft: a power of two, 8 .. 2^20, else DASP_ERR_UNSUPPORTED;  tw: 4096 complex twiddles from dasp_mrstft_table;
 *   work: dasp_fdfir_work_floats(...) floats of scratch (0 up to n_fft = 8192: one launch per direction; -1: unsupported arguments),
 *   its size passed as work_floats (checked: DASP_ERR_ARG). The forward call needs the frames of x only:
 *   2 * h_rows * ((rows / h_rows + 1) / 2) * n_fft floats, one complex frame per two rows of an item.
 *   dasp_fdfir_backward: gx and / or gH may be NULL (skipped); x may be NULL when gH is.
 *   Rows that share a transform: where chs >= 2 rows share a response, rows 2f and 2f + 1 of an item travel as ONE complex frame
 *   x[2f] + i x[2f + 1] (an odd last row, and every row when h_rows = rows, travels alone). Guaranteed: (1) a non-finite sample in a row of
 *   x makes y of that row AND of the row paired with it non-finite at every sample, and gH of the item non-finite (the same for gy and
 *   gx); unpaired rows of the item, every other item, and the outputs the value does not enter (gx for x, y for gy) keep every bit.
 *   (2) The error of a row is bounded relative to the larger peak of its PAIR, not to its own: 2e-5 of the item's largest output peak
 *   (the bound of tests/test_gpu_freqdomain_fir.py); a channel 80 dB below its partner carries the partner's rounding error, 2e-7 .. 3e-7 of the
 *   item's peak, i.e. 2e-3 .. 3e-3 of its own (measured). A caller who needs per-row accuracy passes a response per row (h_rows = rows).
 * ------------------------------------------------------------------------------------------- */
long dasp_fdfir_work_floats(long rows, long T, long n_fft, long h_rows);
int dasp_fdfir_forward(const float* x, const void* H, const void* tw, float* y, float* work, long work_floats, long rows, long T, long n_fft,
                       long h_rows, void* stream);
int dasp_fdfir_backward(const float* x, const void* H, const float* gy, const void* tw, float* gx, void* gH, float* work, long work_floats,
                        long rows, long T, long n_fft, long h_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Level metering and normalisation (csrc/loudness.hip).
 * Integrated loudness of ITU-R BS.1770-4 / EBU R128: K-weighting designed from the sample rate, 400 ms blocks every 100 ms,
 * the absolute gate at -70 LUFS and the relative gate 10 LU below the gated mean; its gradient with the gates held fixed.
 *   x, gx, ysave: (items, chs, N) fp32, rows 4-byte aligned;  1 <= chs <= 5 in the order L R C Ls Rs (weights 1 1 1 1.41 1.41);
 *   8000 <= sample_rate <= 384000;  N >= one block (4 H, H = round(0.1 sample_rate)) and N <= 2^30, else DASP_ERR_UNSUPPORTED.
 *   dasp_loudness_kweighting: the two sections as rows [b0 b1 b2 a0 a1 a2] (12 doubles, host memory) - the table the kernels use.
 *   dasp_loudness_blocks: complete blocks of N samples;  dasp_loudness_segments: workgroups a row of N samples is cut into when there
 *   are `rows` = items * chs of them (1: one workgroup per row; more: a state pre-pass runs first);  -1: unsupported arguments.
 *   scratch: dasp_loudness_scratch_doubles(...) doubles, uninitialised; the backward call takes the same size.
 *   L: (items) LUFS, -inf for an empty gate.  ysave, cov: both NULL (value only), or the K-weighted signal (items, chs, N) and the
 *   coverage weights (items, chs, blocks + 3) kept for dasp_loudness_backward;  gL: (items) upstream gradient.
 *   No atomics, nothing to zero, no host synchronisation: bit-identical run to run, plain kernel nodes under capture.
 *   Non-finite samples: the gates are IEEE comparisons on the block powers, so a block that holds a NaN (every block from a NaN or
 *   +-inf sample on: the filter is recursive) passes neither gate and is left out - L is finite where clean blocks remain, -inf where
 *   none does; it is never read as silence inside a block that counts. The gradient of the ROW that holds the sample is NaN throughout
 *   whenever L is finite (NaN x a coverage weight of 0, filtered backwards over the row; a NaN in the ignored tail too), the item's other
 *   rows stay finite; a NaN gL makes the item's gradient NaN. An item with an empty gate (L = -inf) has a gradient of exactly 0,
 *   whatever its samples and gL hold: the forward call marks it with -0.f throughout its rows of cov, and the backward call then reads
 *   neither ysave nor gL for it. A sample whose square leaves float32 (|K-weighted x| > 1.8e19) is summed in fp64: L is finite (1e30
 *   reads +567 LUFS); the coverage weights are fp32 (about 1 / (block power x 4 H)): beyond some +340 LUFS they turn denormal and
 *   then 0, and so does the gradient. Other items keep every bit.
 * Peak normalisation per row: y = x 10^(peak_db / 20) / max(max |x|, eps);  peak: (rows, 2) doubles written by the forward call
 * (the maximum and the lowest index attaining it) and read by the backward call;  scratch: dasp_peaknorm_scratch_doubles(...) doubles.
 *   A row that holds a NaN has a NaN peak, as torch.max has (peak = (NaN, index of the first NaN)): y and gx of that row are NaN
 *   throughout. A +-inf sample: y is 0 with a NaN at the sample, gx 0 with a NaN at the index of the maximum. eps = 0 on a row of zeros:
 *   y is NaN (0 / 0) and gx +-inf. The constant branch of the gradient is taken for peak <= eps (a peak equal to eps included).
 * ------------------------------------------------------------------------------------------- */
int dasp_loudness_kweighting(double sample_rate, double* sos12);
long dasp_loudness_blocks(long N, double sample_rate);
long dasp_loudness_segments(long rows, long N);
long dasp_loudness_scratch_doubles(long items, int chs, long N, double sample_rate);
int dasp_loudness_forward(const float* x, double* scratch, float* L, float* ysave, float* cov, long items, int chs, long N,
                          double sample_rate, void* stream);
int dasp_loudness_backward(const float* ysave, const float* cov, const float* gL, double* scratch, float* gx, long items, int chs, long N,
                           double sample_rate, void* stream);
long dasp_peaknorm_scratch_doubles(long rows, long N);
int dasp_peaknorm_forward(const float* x, double* scratch, double* peak, float* y, long rows, long N, double peak_db, double eps,
                          void* stream);
int dasp_peaknorm_backward(const float* x, const float* gy, const double* peak, double* scratch, float* gx, long rows, long N,
                           double peak_db, double eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Double precision.  The reference follows the dtype of its input (`.type_as(x)`, dasp_pytorch/signal.py:113,119,
 * functional.py:211), so float64 tensors mean float64 arithmetic. These entry points are that path for the recurrences and the
 * elementwise effects - the same maps as above evaluated plainly, one thread per row / batch item, sequential in time: meant for
 * validation, torch.autograd.gradcheck and small reference runs, not for throughput (csrc/ref64.hip).
 *   c5: (Bs, S, 5) fp64 normalised coefficients [b0 b1 b2 a1 a2] (from dasp_sos64_normalize, or rows of dasp_biquad_design's ba);
 *   wsave: (B*C, S, N) doubles written by the forward pass for the coefficient gradients (NULL when none are wanted);
 *   gc5: (Bs, S, 5) gradient w.r.t. c5, mapped by dasp_sos64_grads to sos (mode 0) or to (gain_db, cutoff_freq, q_factor) (mode 1,
 *   jac = the (Bs, S, 15) Jacobians of dasp_biquad_design);  gsave: (B, N) smoothed gain kept by dasp_dynamics64_forward.
 * ------------------------------------------------------------------------------------------- */
int dasp_sos64_normalize(const double* sos, int Bs, int S, double* c5, void* stream);
int dasp_sos64_forward(const double* c5, int Bs, const double* x, double* y, double* wsave, int B, int C, long N, int S, void* stream);
int dasp_sos64_backward(const double* c5, int Bs, const double* gy, const double* wsave, double* gx, double* gc5, int B, int C, long N,
                        int S, void* stream);
int dasp_sos64_grads(const double* c5, const double* sos, const double* gc5, const double* jac, int Bs, int S, int mode, double* out,
                     void* stream);
int dasp_dynamics64_forward(int mode, const double* x, const double* ctl, double* y, double* gsave, int B, int C, long N,
                            double sample_rate, double eps, int lookahead, void* stream);
int dasp_dynamics64_backward(int mode, const double* x, const double* ctl, const double* gy, const double* gsave, double* gx,
                             double* gctl, int B, int C, long N, double sample_rate, double eps, int lookahead, void* stream);
/* op 0: gain (ctl: B values), op 1: distortion (ctl: B*C values) */
int dasp_ew64_forward(int op, const double* x, const double* ctl, double* y, int B, int C, long N, void* stream);
int dasp_ew64_backward(int op, const double* x, const double* ctl, const double* gy, double* gx, double* gctl, int B, int C, long N,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * The reverb's white noise as the reference draws it.  Replaces `torch.randn(bs*2, 12, num_samples + num_bandpass_taps - 1)`
 * on the global CPU generator (dasp_pytorch/functional.py:548) by the same stream generated on the device: at::mt19937 run from
 * the state the host hands over, one 24-bit float per word, torch's 16-wide Box-Muller layout with its tail rule
 * (csrc/mtrand.hip; host side - state parsing, jump-ahead table - dasp_pytorch_amd/_mt19937.py).
 *   state_host: the 624 words of the generator (host memory, read during the call);  left: its `left` field (1..624);
 *   out: n >= 16 floats (device);  table: the (262, row stride) uint16 jump table on the device, laid out as dasp_mt_layout says
 *   (out8 = {regenerations per unit, baby polynomials, giant polynomials, exponents per uint16 (bit s of word k of a row = the
 *   coefficient of t^(16 k + s)), row stride, window length, max units per call, 0});
 *   scratch: dasp_mt_scratch_words(left, n) 32-bit words (device); after the stream has run, words [*final_state_offset_words, + 624)
 *   hold the generator's words after the draw (when *regenerated != 0; else they are unchanged and not written) and *left_after its
 *   `left`. One call takes at most dasp_mt_max_values() values (a caller with more loops over pieces that are multiples of 16).
 * ------------------------------------------------------------------------------------------- */
int dasp_mt_layout(int* out8);
long long dasp_mt_max_values(void);
long dasp_mt_scratch_words(int left, long long n);
int dasp_mt_randn(const unsigned* state_host, int left, float* out, long long n, const unsigned short* table, unsigned* scratch,
                  int* left_after, int* regenerated, long* final_state_offset_words, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DASP_HIP_H */
