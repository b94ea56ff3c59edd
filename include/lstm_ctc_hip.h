/*
 * lstm_ctc_hip.h — C ABI of liblstm_ctc_hip.so, the MI355X (gfx950) implementation of the
 * mobvoi/lstm_ctc training/inference hot path.
 *
 * The reference has NO plugin/FFI boundary (pure Python 2 + TensorFlow 1.8);
 * each entry point below replaces the TensorFlow op(s) the reference calls at the cited
 * file:line.  A maintainer binds these with ctypes from the nnet package.
 *
 * Conventions
 *   - plain C types; every pointer is a DEVICE pointer owned by the caller unless marked "host";
 *   - the library allocates nothing the caller can see (workspaces are sized by *_workspace_bytes);
 *   - every launch goes to the caller's hipStream_t (passed as void*), asynchronously;
 *   - return 0 on success, negative LC_E* on failure; lc_last_error() gives a thread-local message;
 *   - activations are TIME-MAJOR [T,B,*] float32 (the layout tf.nn.ctc_loss consumes at
 *     nnet/graph.py:72), labels are flat int32 + offsets[B+1] (the SparseTensor of graph.py:76-104).
 */
#ifndef LSTM_CTC_HIP_H
#define LSTM_CTC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC_OK 0
#define LC_EINVAL (-1)   /* bad argument / unsupported shape */
#define LC_ELAUNCH (-2)  /* HIP launch or runtime failure */
#define LC_EWORKSPACE (-3)

typedef void *lc_stream_t; /* hipStream_t */

const char *lc_last_error(void);
int lc_version(void);

/* Development switches.  Each has an LC_* environment variable (read on every call) and a PER-THREAD override that
 * wins over it; LC_OPTION_UNSET clears the override.  lc_get_option returns the effective value (override, else
 * environment, else LC_OPTION_UNSET = "library default").  Names / variables:
 *   "lstm_persistent"  LC_LSTM_PERSISTENT   0 = every recurrence runs the per-step launch train
 *   "lstm_spin_limit"  LC_LSTM_SPIN_LIMIT   bound of the persistent kernels' waits, in polls
 *   "gemm_f32_big"     LC_GEMM_F32_BIG      0 = never the 256 x 256 LDS-DMA kernel, 2 = whenever eligible
 *   "gemm_bf16_big"    LC_GEMM_BF16_BIG     0 = never the 256 x 256 bf16 kernel
 *   "ctc_lse2"         LC_CTC_LSE2          lc_ctc_loss with a gradient: 1 = the per-frame log-sum-exp is taken by phase 2's
 *                                           frame waves (one logits read less; default from 512 utterances), 0 = by phase 1's
 * No reference counterpart (the reference has no native code). */
#define LC_OPTION_UNSET (-0x7fffffffL - 1)
int lc_set_option(const char *name, long value);
int lc_get_option(const char *name, long *value);

/* ------------------------------------------------------------------ CTC --------------------- */
/* tf.nn.ctc_loss(labels, inputs, sequence_length, ignore_longer_outputs_than_inputs=True)
 * as called at nnet/graph.py:109-114 (blank = V-1, ctc_merge_repeated=True).
 *   logits [T,B,V]; labels flat int32; label_offsets [B+1]; seq_len [B];
 *   max_label_len: host-side max_b (offsets[b+1]-offsets[b]);
 *   loss [B] (= -log p; 0 for skipped utterances, +inf when no valid path);
 *   grad [T,B,V] or NULL (d sum(loss) / d logits; 0 beyond seq_len).
 * Shapes: T, B > 0, V >= 2, 0 <= max_label_len <= 1023; with a gradient V <= 10240 (alphabets above 128 classes keep four
 * rows of per-class sums in LDS, 16 V bytes of the 160 KB a workgroup can hold; a loss-only call has no such limit).
 * Anything else or a NULL required pointer is LC_EINVAL, a workspace below lc_ctc_workspace_bytes LC_EWORKSPACE; both
 * launch nothing and leave loss and grad untouched.  Every element of loss and grad is written by a successful call,
 * whatever the workspace held before. */
size_t lc_ctc_workspace_bytes(int T, int B, int V, int max_label_len);
int lc_ctc_loss(const float *logits, int T, int B, int V, const int *labels,
                const int *label_offsets, const int *seq_len, int max_label_len, float *loss,
                float *grad, void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* tf.nn.ctc_greedy_decoder(inputs, sequence_length, merge_repeated=True) — nnet/graph.py:138-142.
 *   tokens [B,T] int32 (row b holds out_len[b] tokens), out_len [B] int32,
 *   workspace: T*B int32 (per-frame argmax). */
int lc_ctc_greedy(const float *logits, int T, int B, int V, const int *seq_len, int *tokens,
                  int *out_len, int *argmax_workspace, lc_stream_t stream);

/* CTC forced alignment: the best (Viterbi) path through the same 2L+1 lattice lc_ctc_loss sums over.  No reference
 * counterpart (TF 1.8 has no such op).  Conventions of lc_ctc_loss: logits [T,B,V] time-major fp32, labels flat int32 +
 * label_offsets [B+1], blank = V-1, ctc_merge_repeated transitions (stay, s-1, and s-2 only onto a non-blank that differs
 * from the label two positions back); the path starts in position 0 or 1 and ends in S-1 or S-2 (S = 2L+1).
 *   ali [B,T]          symbol per frame (blank = V-1); -1 for t >= seq_len[b] and for utterances without a path;
 *   label_index [B,T]  index into utterance b's label sequence; -1 on blank frames and wherever ali is -1; may be NULL;
 *   score [B]          max over paths of sum_t log_softmax(logits[t,b,:])[path_t], natural log; -inf without a path
 *                      (more labels than frames, or too few frames for the blanks between repeated labels - not an
 *                      error); 0 for seq_len 0.  L = 0 gives the all-blank path.
 * Every element of ali, label_index and score is written on every call (no memset needed); the result is deterministic
 * and bit-identical from call to call.  Arithmetic: a cell's emission is the fp32 log-softmax (fp32 log-sum-exp per frame);
 * the sums along paths are carried in double.  Tie rule (exact comparisons): at a cell stay is preferred over s-1 over
 * s-2; at the end S-1 over S-2.  Shapes: whatever lc_ctc_loss accepts (T, B > 0, V >= 2, 0 <= max_label_len <= 1023);
 * anything else is LC_EINVAL with no launch, a workspace below lc_ctc_align_workspace_bytes is LC_EWORKSPACE.  Labels must
 * lie in [0, V-1); an utterance with more labels than max_label_len gets no path. */
size_t lc_ctc_align_workspace_bytes(int T, int B, int V, int max_label_len);
int lc_ctc_align(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                 const int *seq_len, int max_label_len, int *ali, int *label_index, float *score,
                 void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* Alignment-windowed CTC: lc_ctc_loss summed only over the paths that keep every label inside a window of frames - the
 * criterion that bounds emission times with the alignment lc_ctc_align writes.  No reference counterpart.  Everything not
 * said here is lc_ctc_loss's contract (logits [T,B,V] time-major fp32, flat int32 labels + label_offsets [B+1], blank = V-1,
 * ctc_merge_repeated transitions, a path starts in position 0 or 1 and ends in S-1 or S-2, grad may be NULL).
 *   win_lo, win_hi  device int32, parallel to labels: label j of utterance b may occupy frame t only when
 *                   win_lo[j] <= t <= win_hi[j].  Blank positions are never constrained.  Values outside [0, seq_len[b])
 *                   are legal and clip ("unconstrained" is lo <= 0, hi >= T-1); lo > hi is a label with no frame: no path.
 *   loss [B]        -log of the total softmax probability of the surviving paths, natural log;
 *   grad [T,B,V]    softmax - occupancy over the surviving paths on live frames, +0 for t >= seq_len[b]; un-normalised.
 * Conventions of lc_ctc_loss: more labels than frames or seq_len <= 0 -> loss 0, gradient 0; a label outside [0, V-1) (or
 * more labels than max_label_len) -> loss NaN, gradient 0; no surviving path (labels do not fit, an empty window, windows no
 * monotone path satisfies) -> loss +inf, gradient = softmax on the live frames, no NaN anywhere; L = 0 -> the all-blank path.
 * Every element of loss and grad is written on every call (no memset needed); results are bit-identical from call to call
 * (no atomics, fixed summation orders).  Arithmetic: fp32 log-softmax emissions; the lattice cells are doubles in the log2
 * domain (the log-sum-exp of a cell's predecessors on the fp32 exp2 / log2 pipes relative to their maximum, the additions
 * in double), so a cell's error does not grow with its magnitude; log p and the occupancy exponents are formed in double
 * and rounded once.
 * Shapes: lc_ctc_loss's (T, B > 0, V >= 2, 0 <= max_label_len <= 1023); anything else or a NULL required pointer is
 * LC_EINVAL with no launch, a workspace below lc_ctc_window_workspace_bytes (0 for a bad shape) is LC_EWORKSPACE.  Elements
 * are indexed in 64 bits.  The workspace holds both lattices: about 2 * T * B * roundup(2 * max_label_len + 1, 64) doubles. */
size_t lc_ctc_window_workspace_bytes(int T, int B, int V, int max_label_len);
int lc_ctc_loss_windowed(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                         const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi,
                         float *loss, float *grad, void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* Delay-penalised CTC (Kang et al. 2023): the CTC criterion over paths weighted by exp(-delay_penalty * E(path)), E(path) =
 * sum over the labels of the first frame of the label's run - "emit earlier" without an alignment - and the expectation of E
 * under that weighted path posterior.  No reference counterpart.  Everything not said here is lc_ctc_loss_windowed's contract.
 *   win_lo, win_hi  both NULL = unconstrained; else lc_ctc_loss_windowed's windows (exactly one NULL is LC_EINVAL);
 *   delay_penalty   lambda, any finite value (not finite -> LC_EINVAL); 0 is plain (windowed) CTC.  The weight sits on the
 *                   ARCS that enter a label position (from s-1 or s-2) at frame t, exp(-lambda * t), not centred: frame 0
 *                   carries none, "stay" arcs and arcs into blanks carry none, so loss >= the unpenalised loss for lambda >= 0;
 *   loss [B]        -log sum_path p(path | x) exp(-lambda E(path)), natural log;
 *   entry_sum [B]   or NULL: E_q[E(path)], q(path) ~ p(path | x) exp(-lambda E(path)) = d loss / d lambda = sum_t sum_s
 *                   occupancy(t, s) * (L - (s + 1) / 2).  entry_sum / L is the mean frame at which a label is entered;
 *   grad [T,B,V]    or NULL: softmax - occupancy under q on live frames, +0 for t >= seq_len[b].
 * lc_ctc_loss's conventions: a skipped utterance -> loss 0, entry_sum 0, gradient 0; a bad label -> loss NaN, entry_sum NaN,
 * gradient 0; no surviving path -> loss +inf, entry_sum 0, gradient = softmax, no NaN anywhere; L = 0 -> the all-blank path
 * (entry_sum 0).  Every element of every output is written on every call; results are bit-identical from call to call and
 * loss is bit-identical whichever of entry_sum / grad are NULL (no atomics, fixed summation orders).  A non-NULL entry_sum
 * runs both sweeps also without a gradient.  Arithmetic: lc_ctc_loss_windowed's (fp32 log-softmax emissions, double cells
 * in the log2 domain); the arc weight -lambda * log2(e) * t is formed and added in double; log p, the occupancy exponents and
 * entry_sum (per-frame terms in the workspace, folded per utterance in a fixed order) are formed in double and rounded once.
 * Shapes and errors as for lc_ctc_loss_windowed; the workspace holds T * B doubles more. */
size_t lc_ctc_delay_workspace_bytes(int T, int B, int V, int max_label_len);
int lc_ctc_loss_delay(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                      const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi, float delay_penalty,
                      float *loss, float *entry_sum, float *grad, void *workspace, size_t workspace_bytes,
                      lc_stream_t stream);

/* Maximum-entropy CTC (EnCTC; Liu, Jin and Zhang, NeurIPS 2018): the CTC loss, the entropy of the posterior over the feasible
 * paths, and the gradient of loss - entropy_weight * entropy.  No reference counterpart.  Everything not said here is
 * lc_ctc_loss_windowed's contract (blank = V-1, ctc_merge_repeated transitions, a path starts in position 0 or 1 and ends in
 * S-1 or S-2).  With log p(pi) = sum_t log_softmax(logits[t,b,:])[pi_t], Z = sum_pi p(pi) over the feasible paths and
 * Ebar = sum_pi (p(pi) / Z) log p(pi):
 *   win_lo, win_hi  both NULL = unconstrained; else lc_ctc_loss_windowed's windows (exactly one NULL is LC_EINVAL);
 *   entropy_weight  eta, any finite value (not finite -> LC_EINVAL); it enters the gradient only;
 *   loss [B]        -log Z, natural log: exactly lc_ctc_loss_windowed's loss with windows and lc_ctc_loss_delay's at
 *                   delay_penalty 0 without, bit for bit;
 *   entropy [B]     required: H = -sum_pi (p / Z) log(p / Z) = log Z - Ebar in nats; >= 0, +0 exactly when one path survives;
 *   grad [T,B,V]    or NULL: d (loss - eta H) / d logits, the exact derivative (nothing is held constant) =
 *                   softmax - sum_{s: class(s) = k} occupancy(t, s) (1 + eta (Ebar - c(t, s))), c(t, s) the mean of log p(pi)
 *                   over the posterior restricted to the paths through (t, s); live rows still sum to 0; +0 for
 *                   t >= seq_len[b].  With entropy_weight 0 it is those siblings' grad, bit for bit.
 * lc_ctc_loss's conventions: a skipped utterance -> loss 0, entropy 0, gradient 0; a bad label -> loss NaN, entropy NaN,
 * gradient 0; no surviving path -> loss +inf, entropy 0, gradient = softmax, no NaN anywhere; L = 0 -> the all-blank path,
 * entropy +0.  Every element of every output is written on every call; results are bit-identical from call to call and
 * loss / entropy are bit-identical with and without a gradient (no atomics, fixed summation orders).  Without a gradient
 * only the forward sweep runs.  Arithmetic: lc_ctc_loss_windowed's cells, and beside each cell a double m = the mean of
 * log2 p over the prefixes that end in it (the expectation semiring's second component): emission + the mean of the
 * predecessors' m under the weights the cell's log-sum-exp forms, taken relative to the heaviest predecessor's m, so that
 * the error is a few fp32 ulps of the spread of the m, not of their size, and a single path is carried exactly; m is a
 * plain number, 0 in a dead cell.  Ebar, H = (log2 Z - Ebar) ln 2 and the gradient's occupancy * (Ebar - c) terms (each
 * formed as that product, summed per class in the plain gradient's order) are in double and rounded once.
 * Shapes and errors as for lc_ctc_loss_windowed; the workspace holds both lattices twice (cells and means). */
size_t lc_ctc_entropy_workspace_bytes(int T, int B, int V, int max_label_len);
int lc_ctc_loss_entropy(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                        const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi,
                        float entropy_weight, float *loss, float *entropy, float *grad,
                        void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* Transcript-tolerant CTC (after OTC / BTC, Gao et al. 2023, and STC, Pratap et al. 2022): the CTC criterion on a lattice whose
 * every position may explain a frame by a penalised star symbol, "some non-blank class", instead of by its own class, and
 * the expected number of frames the star explains.  No reference counterpart.  Everything not said here is
 * lc_ctc_loss_windowed's contract (blank = V-1, ctc_merge_repeated transitions, a path starts in position 0 or 1 and ends in
 * S-1 or S-2).  With q = softmax(logits[t,b,:]), Qnb(t) = sum_{k < V-1} q_k and qstar(t) = Qnb(t) / (V - 1), the emission of
 * lattice position s at frame t is the mixture e'(t, s) = q_y(t) + exp(-bypass_penalty) qstar(t) at a label position of
 * class y (the label may be bypassed: a substituted or inserted label) and q_blank(t) + exp(-selfloop_penalty) qstar(t) at a
 * blank position (the blank may absorb speech: a deleted label); Z = sum over the feasible paths of prod_t e'(t, s_t):
 *   win_lo, win_hi  both NULL = unconstrained; else lc_ctc_loss_windowed's windows (exactly one NULL is LC_EINVAL);
 *   bypass_penalty, selfloop_penalty  each >= 0 or +inf (NaN, negative, -inf -> LC_EINVAL, nothing is launched); +inf
 *                   switches that star off;
 *   loss [B]        -log Z, natural log.  It MAY BE NEGATIVE: e' is not normalised over the classes;
 *   star_frames [B] required: sum_t M(t), M(t) = sum_s occupancy(t, s) sigma(t, s), sigma = the star's share of e': the
 *                   expected number of frames explained by the star under the path posterior; equally d loss / d p when
 *                   both penalties move together, and loss is concave in that p;
 *   grad [T,B,V]    or NULL: softmax_k - rho_k occ_k - [k < V-1] (q_k / Qnb) M(t), rho = the own share of e', occ_k the
 *                   occupancy of class k's positions: the exact derivative; live rows sum to 0; +0 for t >= seq_len[b].
 * With both penalties +inf, loss and grad are lc_ctc_loss_windowed's (with windows) and lc_ctc_loss_delay's at delay_penalty 0
 * (without), bit for bit, and star_frames is +0.
 * lc_ctc_loss's conventions: a skipped utterance -> loss 0, star_frames 0, gradient 0; a bad label -> loss NaN, star_frames
 * NaN, gradient 0; no surviving path -> loss +inf, star_frames 0, gradient = softmax, no NaN anywhere; L = 0 -> the all-blank
 * path, whose cells still carry the self-loop star.  A frame whose non-blank logits are all -inf has no star.  Every element
 * of every output is written on every call; results are bit-identical from call to call and loss / star_frames are
 * bit-identical with and without a gradient (no atomics, fixed summation orders; both sweeps always run).
 * This is a per-frame mixture, not OTC's WFST: there the star is a separate arc that replaces a label and is then followed
 * by that star's own self-loops; here the star is an alternative of the CELL at every single frame, so a run of frames in
 * one position may switch between own class and star frame by frame, the transitions are plain CTC's, and no graph is
 * composed.  Arithmetic: lc_ctc_loss_windowed's double cells in the log2 domain; the star term is
 * (lse_nb - lse) log2 e - log2(V - 1) - penalty log2 e with lse_nb a second fp32 log-sum-exp over the non-blank classes
 * (never log(1 - q_blank)), the constant part formed in double and rounded once; e' = max + log2(1 + 2^-|difference|) on the
 * fp32 pipes; M(t) and its fold in double, rounded once.
 * Shapes and errors as for lc_ctc_loss_windowed; the workspace is lc_ctc_loss_delay's plus T * B floats. */
size_t lc_ctc_star_workspace_bytes(int T, int B, int V, int max_label_len);
int lc_ctc_loss_star(const float *logits, int T, int B, int V, const int *labels, const int *label_offsets,
                     const int *seq_len, int max_label_len, const int *win_lo, const int *win_hi,
                     float bypass_penalty, float selfloop_penalty, float *loss, float *star_frames, float *grad,
                     void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* Frame-level softmax cross-entropy against one target symbol per frame - the objective that trains on what lc_ctc_align
 * writes.  No reference counterpart (the reference never finished frame-level training).
 *   logits [T,B,V] time-major fp32; targets [B,T] int32 (the layout of lc_ctc_align's ali); seq_len [B].
 * A frame (t, b) is SCORED when t < seq_len[b] and 0 <= targets[b,t] < V.  Class V-1 (the blank) is a legal target here;
 * -1 means "ignore".
 *   loss [B]     sum over scored frames of -log_softmax(logits[t,b,:])[target], natural log;
 *   frames [B]   number of scored frames;
 *   correct [B]  scored frames whose argmax equals the target (lowest index among equal maxima: lc_ctc_greedy's rule);
 *   grad [T,B,V] or NULL: d sum_b loss[b] / d logits = softmax - onehot on scored rows, +0 on every other row;
 *                un-normalised, the convention of lc_ctc_loss.
 * A live target < -1 or >= V makes loss[b] NaN (lc_ctc_loss's convention for bad labels); its frame counts nowhere and gets
 * a zero row.  -inf logits behave as in float arithmetic: a -inf non-target class contributes 0 and gets gradient 0, a -inf
 * target gives +inf loss, an all -inf row gives NaN.
 * Every element of loss, frames, correct and grad is written on every call (no memset needed); results are bit-identical
 * from call to call (no atomics: the per-frame terms go to the workspace - 8 bytes per frame - and a second launch folds
 * each utterance's terms in a fixed order in double and rounds once to float).  Arithmetic per frame: one fp32 log-sum-exp
 * and one fp32 subtraction.  Rows of V <= 1024 are read once and kept in registers up to the gradient store (V <= 64: four
 * frames per wave); wider rows are re-read.  T, B <= 0, V < 2 or a NULL required pointer: LC_EINVAL with no launch; a
 * workspace below lc_xent_workspace_bytes: LC_EWORKSPACE.  Elements are indexed in 64 bits (T * B * V may exceed 2^31). */
size_t lc_xent_workspace_bytes(int T, int B, int V);
int lc_xent_loss(const float *logits, int T, int B, int V, const int *targets, const int *seq_len, float *loss,
                 int *frames, int *correct, float *grad, void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* Teacher-student distillation: per-frame KL divergence from a teacher's whole posterior to the student's, the soft-target
 * relative of lc_xent_loss.  No reference counterpart.
 *   logits  [T,B,V] time-major fp32, the student, as lc_xent_loss takes them;
 *   teacher [T,B,V] teacher scores in the LOG domain (logits or log-posteriors: a per-row constant shift is immaterial;
 *           -inf = probability 0);  seq_len [B];  teacher_len [B]: frames of utterance b that carry a teacher row.
 * A frame (t, b) is SCORED when t < seq_len[b] and t < teacher_len[b].  With p = softmax(teacher / tau) and q =
 * softmax(logits / tau), tau = temperature > 0:
 *   loss [B]     sum over scored frames of KL(p || q) = sum_k p_k (log p_k - log q_k), natural log, p_k = 0 -> term 0;
 *                NOT scaled by grad_scale and NOT clamped (a KL that rounds below zero stays there);
 *   frames [B]   number of scored frames;
 *   agree [B]    scored frames whose two argmaxes coincide (lowest index among equal maxima on both rows);
 *   grad [T,B,V] or NULL: grad_scale * (q - p) on scored rows.  accumulate == 0: stored, every other row +0; accumulate != 0:
 *                added to what grad holds, every other row left bit-exactly as it was (neither read nor written).
 * The caller passes grad_scale = lambda * tau: the derivative of lambda * tau^2 * KL with respect to the logits.
 * A teacher row whose maximum is not finite (all -inf, a +inf) or that holds a NaN makes loss[b] NaN; its frame counts
 * nowhere and adds nothing to grad (a zero row when storing).  A student -inf where p_k > 0 gives +inf loss and a finite
 * gradient row; student rows that are not finite behave as in lc_xent_loss.  An unscored frame's two rows are never read.
 * Every element of loss, frames and agree (and of grad when storing) is written on every call; results are bit-identical
 * from call to call and with and without a gradient (no atomics: 8 bytes per frame go to the workspace and a second launch
 * folds each utterance's terms in a fixed order in double, rounding once).  Arithmetic per frame, fp32: both maxima are
 * taken out first (a = s - max s, b = z - max z), then KL = sum_{p_k > 0} exp(a_k / tau) (a_k - b_k) / (tau Sp) + ln Sq - ln Sp
 * with Sp, Sq the two sums of exponentials - no per-element log.  Rows of V <= 1024 are read once and kept in registers up
 * to the gradient store (V <= 64: four frames per wave); wider rows are re-read.  T, B <= 0, V < 2, a temperature that is not
 * finite and > 0, or a NULL required pointer: LC_EINVAL with no launch; a workspace below lc_kd_workspace_bytes:
 * LC_EWORKSPACE; both leave every output alone.  Elements are indexed in 64 bits (T * B * V may exceed 2^31). */
size_t lc_kd_workspace_bytes(int T, int B, int V);
int lc_kd_loss(const float *logits, const float *teacher, int T, int B, int V, const int *seq_len, const int *teacher_len,
               float temperature, float grad_scale, float *loss, int *frames, int *agree, float *grad, int accumulate,
               void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* Consistency-regularised CTC (CR-CTC): the per-frame symmetric KL between the posteriors of two views of one utterance
 * that sit in the two halves of ONE batch - lc_kd_loss's sibling, reading each row once.  No reference counterpart.
 *   B       the number of PAIRS;
 *   logits  [T,2B,V] time-major fp32: row (t, b) is view a of pair b, row (t, b + B) is view b;
 *   seq_len [B] one length per pair.  A pair-frame (t, b) is SCORED when t < seq_len[b].
 * With qa = softmax(za) and qb = softmax(zb) (natural log, no temperature):
 *   loss [B]      sum over scored pair-frames of J = KL(qb || qa) + KL(qa || qb) = sum_k (qa_k - qb_k)(log qa_k - log qb_k);
 *                 a class with probability 0 in both views contributes 0; NOT scaled by grad_scale and NOT clamped;
 *   frames [B]    number of scored pair-frames;
 *   agree [B]     scored pair-frames whose two argmaxes coincide (lowest index among equal maxima, lc_ctc_greedy's rule);
 *   grad [T,2B,V] or NULL: on scored pair-frames row a gets grad_scale * (qa - qb) and row b grad_scale * (qb - qa).  This is
 *                 the STOP-GRADIENT form - each view is a constant target for the other - and therefore NOT the derivative
 *                 of J (it is that of KL(qb || qa) in za with qb held fixed, and of KL(qa || qb) in zb with qa held fixed).
 *                 accumulate == 0: stored, every other row +0; accumulate != 0: added to what grad holds, every other row
 *                 left bit-exactly as it was (neither read nor written).
 * A row of EITHER view whose maximum is not finite (all -inf, a +inf) or that holds a NaN makes loss[b] NaN; its pair-frame
 * counts nowhere and adds nothing to grad (two zero rows when storing).  A finite row with -inf entries behaves as float
 * arithmetic gives: qa_k > 0 against zb_k = -inf is +inf loss and finite gradient rows.  An unscored pair-frame's rows are
 * never read.  Every element of loss, frames and agree (and of grad when storing) is written on every call; results are
 * bit-identical from call to call and with and without a gradient (no atomics: 8 bytes per pair-frame go to the workspace
 * and a second launch folds each pair's terms in a fixed order in double, rounding once).  Arithmetic per pair-frame, fp32:
 * a = za - max za, b = zb - max zb, d_k = exp(a_k) / Sa - exp(b_k) / Sb with Sa, Sb the two sums of exponentials, J =
 * sum_{d_k != 0} d_k ((a_k - b_k) - (ln Sa - ln Sb)) - no per-element log, and exactly 0 (with a zero gradient) for two equal
 * rows.  Rows of V <= 1024 are read once and kept in registers up to the gradient stores (V <= 64: four pair-frames per
 * wave); wider rows are re-read.  T, B <= 0, V < 2, a grad_scale that is not finite, a NULL required pointer, or accumulate
 * != 0 with grad == NULL: LC_EINVAL with no launch; a workspace below lc_consistency_workspace_bytes: LC_EWORKSPACE; both
 * leave every output alone.  Elements are indexed in 64 bits (T * 2B * V may exceed 2^31). */
size_t lc_consistency_workspace_bytes(int T, int B, int V);
int lc_consistency_loss(const float *logits, int T, int B, int V, const int *seq_len, float grad_scale, float *loss,
                        int *frames, int *agree, float *grad, int accumulate, void *workspace, size_t workspace_bytes,
                        lc_stream_t stream);

/* tf.edit_distance(hyp, truth, normalize=False) — nnet/graph.py:143-149.  HOST function on HOST
 * buffers (integer DP on a few hundred tokens; SURVEY.md §2a keeps it on the host). */
int lc_edit_distance_host(const int *hyp, int hyp_stride, const int *hyp_len, const int *truth,
                          const int *truth_offsets, int B, int *dist);

/* ------------------------------------------------------------------ GEMM -------------------- */
/* C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] + beta * C (+ bias[N] broadcast over rows if non-NULL),
 * float32 on the f32 MFMA pipe.  Row-major; ta/tb != 0 means the stored matrix is the transpose
 * (A stored [K,M], B stored [N,K]).  Replaces tf.matmul / tf.nn.xw_plus_b (nnet/bilstm.py:249,
 * nnet/moe.py:43,58) and the batched halves of the LSTMCell kernel matmul (bilstm.py:129-136). */
/* Tall-K products with few output tiles (weight gradients, K = T*B) are split along K into slabs in the
 * caller's workspace (lc_gemm_workspace_bytes; 0 = no split) and reduced deterministically.  A NULL or
 * too-small workspace just disables the split. */
size_t lc_gemm_workspace_bytes(int M, int N, int K);
int lc_gemm_f32(int ta, int tb, int M, int N, int K, float alpha, const float *A, int lda,
                const float *B, int ldb, float beta, float *C, int ldc, const float *bias,
                void *workspace, size_t workspace_bytes, lc_stream_t stream);
/* Same product with bf16 OPERANDS (BASELINE.json configs[4], "bf16 MFMA gate GEMMs, fp32 CTC"): A and B stay
 * float32 in memory and are rounded to bf16 (round-to-nearest-even) as they are loaded,
 *   C = alpha * sum_k bf16(A[m,k]) * bf16(B[k,n]) + beta*C + bias,  accumulated in float32 by
 * v_mfma_f32_32x32x16_bf16.  Outputs, bias, alpha/beta arithmetic stay float32.  Same workspace rule. */
int lc_gemm_bf16(int ta, int tb, int M, int N, int K, float alpha, const float *A, int lda,
                 const float *B, int ldb, float beta, float *C, int ldc, const float *bias,
                 void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* bf16 SHADOW operands (second stage of the c5 path): the activations / weights are first copied to bf16 -
 * lc_cast_bf16 writes the same-orientation copy nat[rows][ldnat] and / or the transposed copy tr[C][ldtr] (either
 * may be NULL) of a float32 x[rows, C] (round-to-nearest-even) - and every product is then taken in "NT" form,
 *   C[M,N] = alpha * sum_k A[m,k] * B[n,k] + beta*C + bias,   A[M][K], B[N][K] bf16 with k contiguous,
 * so the loader is a plain 16-byte copy (no conversion, no transposition).  Bit-identical operands to lc_gemm_bf16
 * (same rounding), float32 accumulate / outputs.  K, lda, ldb multiples of 8; A, B 16-byte aligned. */
int lc_cast_bf16(const float *x, int rows, int C, int ldx, uint16_t *nat, int ldnat, uint16_t *tr, int ldtr,
                 lc_stream_t stream);
int lc_gemm_bf16_nt(int M, int N, int K, float alpha, const uint16_t *A, int lda, const uint16_t *B, int ldb,
                    float beta, float *C, int ldc, const float *bias, void *workspace, size_t workspace_bytes,
                    lc_stream_t stream);
/* Two operand pairs into one result, C = alpha * (A1 B1^T + A2 B2^T) + beta*C + bias, in ONE pass over C (whole 256 x 256
 * tiles: one kernel whose reduction walks K1 then K2; elsewhere the two products one after the other): the input gradient
 * of a bidirectional layer - both cells read the same concatenated input, nnet/bilstm.py:190-203, so TF's gradient pass
 * adds the two tf.matmul(dz, Kx, transpose_b=True) nodes of nnet/bilstm.py:129-136,150-157.  Same operand rules as
 * lc_gemm_bf16_nt; both pairs share lda / ldb.  A fused epilogue (lc_gemm_next_epilogue) applies to the final value. */
int lc_gemm_bf16_nt2(int M, int N, int K1, int K2, float alpha, const uint16_t *A1, const uint16_t *A2, int lda,
                     const uint16_t *B1, const uint16_t *B2, int ldb, float beta, float *C, int ldc, const float *bias,
                     lc_stream_t stream);
/* The same two-pair product in float32 (config c4): A1, A2 [M][K] and B1, B2 [N][K] float32, k contiguous, 16-byte aligned
 * with lda / ldb multiples of 4 for the one-kernel route (K1, K2 multiples of 32, whole 256 x 256 tiles); anything else runs
 * the two lc_gemm_f32 products in sequence.  7.43 + 7.88 ms -> 14.78 ms at c4's dX shape (the second product's beta = 1 pass). */
int lc_gemm_f32_nt2(int M, int N, int K1, int K2, float alpha, const float *A1, const float *A2, int lda,
                    const float *B1, const float *B2, int ldb, float beta, float *C, int ldc, const float *bias,
                    lc_stream_t stream);
/* The same product with BOTH operands K-MAJOR: A stored [K][M], B stored [K][N] (C = alpha * A^T B + beta * C + bias) -
 * the weight gradients X^T dZ of a train step on the NATURAL bf16 shadows of the activations (their rows are the
 * reduction index), so no transposed copy is made.  M and N must be multiples of 256, lda / ldb multiples of 8, any K.
 * Replaces the tf.matmul(..., transpose_a=True) nodes TF's gradient pass builds for nnet/bilstm.py:129-136,249. */
int lc_gemm_bf16_tn(int M, int N, int K, float alpha, const uint16_t *A, int lda, const uint16_t *B, int ldb,
                    float beta, float *C, int ldc, const float *bias, void *workspace, size_t workspace_bytes,
                    lc_stream_t stream);
/* ... and with A k-contiguous [M][K], B K-MAJOR [K][N] (C = alpha * A B + ...): the forward products X . Kx, hs . proj on
 * the natural shadows of activation and weight - no transposed weight copy.  M, N multiples of 256, K of 64. */
int lc_gemm_bf16_nn(int M, int N, int K, float alpha, const uint16_t *A, int lda, const uint16_t *B, int ldb,
                    float beta, float *C, int ldc, const float *bias, void *workspace, size_t workspace_bytes,
                    lc_stream_t stream);

/* One-shot fused epilogue: arms the NEXT lc_gemm_* call of the calling thread (any of the five above; it is consumed by that
 * call whether it succeeds or not) to finish its output element (r, c) of the whole M x N result in the product kernel:
 *   keep < 1:  C[r][c] *= the DropoutWrapper factor of (seed, stream0 + c / drop_width, r * drop_width + c % drop_width) -
 *              bit-identical to lc_dropout_scale(keep, seed, stream0 + d) on each column window d of width drop_width
 *              (nnet/bilstm.py:147-160: one wrapper per direction; its backward applies the same mask to dY);
 *   c_bf16:    the final value, rounded to bf16 (RNE), also goes to c_bf16[r * ldc_bf16 + c] - the shadow operand the next
 *              product reads (what lc_cast_bf16 / lc_dropout_scale_bf16 would write in a pass of their own).
 * An armed product is never split along K (the mask lives in the product kernel), and beta, bias are applied BEFORE the mask.
 * e == NULL disarms.  Replaces the separate tf.nn.dropout node after each direction's projection. */
typedef struct lc_gemm_epilogue {
    float keep;            /* 1.0: no mask */
    uint32_t seed, stream0;
    int drop_width;        /* P: columns per dropout stream */
    uint16_t *c_bf16;      /* or NULL */
    int ldc_bf16;
    int shadow_only;       /* non-zero (needs c_bf16): ONLY the shadow is written; the float32 C is UNSPECIFIED afterwards (left
                            * untouched, except where lc_gemm_bf16_nt2 runs its two products in sequence - ragged edges, small
                            * shapes - and keeps the first one's partial sum there) - for
                            * outputs every later product reads through the shadow (a c5 step's layer outputs and input
                            * gradients): a third of the bytes, and of the store burst that ends every tile */
} lc_gemm_epilogue_t;
int lc_gemm_next_epilogue(const lc_gemm_epilogue_t *e);

/* fp32 products on the bf16 matrix cores ("bf16x3", config key compute_dtype = bf16x3): each fp32 operand element is split
 * exactly into three bf16 terms (hi + mid + lo) by lc_split_bf16x3, and lc_gemm_bf16x3_nt accumulates, in fp32, the six term
 * pairs of weight >= 2^-16 (what is dropped is <= 2^-25 of each product - a quarter of an fp32 ulp).  Same tf.matmul nodes as
 * lc_gemm_f32 (nnet/bilstm.py:129-136,249), fp32-grade results, 6 bf16 MFMAs per 16 k instead of 8 fp32 MFMAs.
 *
 * Range: the split is exact for 1e-30 <= |x| <= 3.38e38 (bf16's largest finite value) and for zero; smaller magnitudes lose
 * their low terms to the fp32 denormal flush (absolute error < 2^-126); Inf, NaN and |x| above bf16's maximum give NaN.
 *
 * Error bound (lc_gemm_bf16x3_nt, _tn, and the split-operand recurrences lc_lstm_fwd_x3 / _bwd_x3), per output element with
 * alpha = 1, beta = 0:
 *     | C - sum_k a_k b_k |  <=  3e-7 * max(1, sqrt(K) / 4) * sum_k |a_k| |b_k|  +  2^-125 * sum_k (|a_k| + |b_k|)
 * The first term is the fp32 accumulation both this product and the fp32 MFMA kernels carry (the dropped term pairs add
 * <= 2^-23 of it); the second is the flush of split terms below 2^-126 and only shows where an operand below ~1e-30 meets one
 * above ~1e+8.  Held by tests/test_gpu_ops.py::test_gemm_bf16x3_adversarial_operands on rows that cancel to 1e-6 of their
 * magnitude sum, per-row magnitude spreads of 2^24, operands in [1e-38, 1e-30], +-0 and fp32 denormals, next to the fp32
 * kernel on the same operands.  At MODEL level the claim is about FLOAT64 TRUTH, not about the fp32 mode: the split-operand
 * mode's logits are as far from a float64 evaluation of the same network as the fp32 kernels' are - measured at the benched
 * sizes with the reference's initialisation (profiles/r5_x3_truth.txt: rms error bf16x3 / fp32 = 0.97 .. 1.07 over
 * N = 320 .. 1024, 1 .. 5 layers, T = 300 .. 1000; tests/test_gpu_truth.py asserts <= 1.5 at N = 128, 512, 768, 1024 with
 * the schedule taken), and per step (profiles/r5_x3_local_error.txt: teacher-forced |dc|, |dh| over a T = 1000 trajectory
 * equal to the fp32 kernel's, 0.3 ulp of c).  The two modes do NOT agree with EACH OTHER on long sequences, and no two fp32
 * implementations do: at forget bias 5 the cell is a 150-step integrator (|c| up to ~650) and a 5-layer, T = 1000 stack
 * amplifies rounding-level differences until fp32 logits are uncorrelated with float64's (rms 0.52 on logits of rms 0.70
 * for the fp32 kernels, 0.52 for bf16x3, 0.45 for an independent fp32 implementation in torch, 0.78 for plain bf16) - so
 * `bf16x3 - fp32` (rms 0.42 at c4's full size) measures the workload's conditioning, not either mode.
 *
 * x3 shadow layout: row-major, row r = [k tile 0: hi[16] mid[16] lo[16] | k tile 1: ... ], K padded with zeros to a multiple
 * of 16; ldo (bf16 elements) >= 3 * roundup(cols, 16), multiple of 8; out 16-byte aligned. */
int lc_split_bf16x3(const float *x, int rows, int cols, int ldx, uint16_t *out, int ldo, lc_stream_t stream);
/* C[M,N] = alpha * A[M,K] * B[N,K]^T + beta * C + bias[N] on x3 shadows (both operands k-contiguous; any M, N, K).  Honours
 * lc_gemm_next_epilogue. */
int lc_gemm_bf16x3_nt(int M, int N, int K, float alpha, const uint16_t *A, int lda, const uint16_t *B, int ldb,
                      float beta, float *C, int ldc, const float *bias, lc_stream_t stream);
/* C[M,N] = alpha * A^T B + beta * C + bias[N] with BOTH operands K-major x3 shadows - A of X [K, M], B of dZ [K, N]: the
 * weight gradients (tf.matmul(..., transpose_a=True) in TF's gradient of nnet/bilstm.py:129-136,249) on the SAME shadows the
 * forward / dX products read as row operands (row windows are fine: dR = hs_prev^T dZ).  Any M, N, K; with a workspace of
 * lc_gemm_bf16x3_tn_workspace_bytes the reduction is split along K (deterministic slices + a reduction pass) so that few
 * output tiles still fill the chip.  A pending lc_gemm_next_epilogue is consumed and ignored. */
size_t lc_gemm_bf16x3_tn_workspace_bytes(int M, int N, int K);
/* The same for operands with the given leading dimensions (row windows of wider shadows): a K slice of an operand is addressed
 * through one buffer descriptor (2 GB reach), so K * max(lda, ldb) * 2 bytes beyond that force more slices - and a workspace -
 * whatever the tile count.  lc_gemm_bf16x3_tn_workspace_bytes(M, N, K) is this with the minimal leading dimensions. */
size_t lc_gemm_bf16x3_tn_workspace_bytes_ld(int M, int N, int K, int lda, int ldb);
int lc_gemm_bf16x3_tn(int M, int N, int K, float alpha, const uint16_t *A, int lda, const uint16_t *B, int ldb,
                      float beta, float *C, int ldc, const float *bias, void *workspace, size_t workspace_bytes,
                      lc_stream_t stream);

/* ------------------------------------------------------------------ LSTM -------------------- */
/* The sequential part of tf.contrib.rnn.LSTMCell under tf.nn.dynamic_rnn with sequence_length
 * masking (nnet/bilstm.py:125-188), for one direction or for both directions
 * of a BiLSTM layer in the same launches.
 *
 * Column layout of every [.,4N] operand is GATE-INTERLEAVED: column (n/8)*32 + g*8 + n%8 holds gate
 * g (0=i,1=j,2=f,3=o) of unit n (TF keeps [i|j|f|o] blocks of N; the host permutes at checkpoint I/O).
 *   zx     [T,B,4N]  in: x_t.Kx + bias; out: activated gates (i, tanh j, f, o)
 *   R      [N,4N]    recurrent weights acting on m' (= proj.Kh with a projection layer, else Kh)
 *   w_f,w_i,w_o [N]  peepholes or NULL
 *   cs, hs [T,B,N]   out: cell state c_t and pre-projection output m'_t (0 where t >= seq_len[b])
 *   reverse != 0     run t = T-1..0: the reference's reverse_sequence -> dynamic_rnn -> reverse_sequence
 *                    (bilstm.py:112,180-190) done by index arithmetic.
 * Requires N % 16 == 0 in both passes of lc_lstm_fwd / lc_lstm_bwd and of the split-operand entry points, and
 * N % 32 == 0 in both passes of the bf16 ones; anything else is refused with LC_EINVAL before any launch. */
typedef struct {
    float *zx;
    const float *R;
    const float *w_f, *w_i, *w_o;
    float *cs, *hs;
    int reverse;
    uint16_t *hs_bf16;   /* lc_lstm_fwd_bf16 only, may be NULL: [T,B,N] bf16 (round-to-nearest-even) copy of hs, written in the
                          * same pass - the shadow operand the next product (m = m'.proj) reads, without a separate cast */
    int shadow_only;     /* lc_lstm_fwd_bf16 with hs_bf16: non-zero = the caller reads hs only through hs_bf16; the float32 hs
                          * is then UNSPECIFIED after the call (the full-width persistent kernel does not store it: one
                          * vector-memory instruction less per step).  zx and cs are written as always. */
} lc_lstm_fwd_dir_t;
/* Stream semantics: everything is ordered after prior work on `stream` and before later work on it.  For the big
 * bidirectional float32 case the reverse direction runs on an internal second stream that is forked from and joined
 * back into `stream` with events inside the call.
 * Schedules (same results up to float32 summation order): num_neurons <= 512, float32 and at most 64 batch rows
 * (128 uni-directional) run as ONE persistent launch per call - one XCD per (direction, row group), weights resident
 * in registers, state exchanged through that XCD's L2 (environment LC_LSTM_PERSISTENT=0 disables it); num_neurons in
 * {640, 768, 896, 1024} in float32 runs persistent launches on XCD PAIRS (the recurrent weights of half the units in each XCD's
 * registers, partial sums handed across): 64 batch rows of both directions - or 128 rows of one direction - per launch,
 * larger batches as consecutive launches over 64-row blocks of the same tensors, as long as T * B * 4N * 4 bytes < 2^32;
 * everything else runs one launch per time step.  The persistent launch needs the GPU's CUs free to become co-resident; every wait in
 * it is bounded, and a timeout writes NaN into the outputs instead of hanging. */
/* Failure reporting of the persistent schedule.  The first 256 bytes of the LSTM workspace are a control block; the
 * 32-bit word at byte LC_LSTM_STATUS_OFFSET is a STICKY status word: the library never clears it, and sets it to a
 * non-zero value when a persistent launch could not complete (a bounded wait ran out - e.g. its workgroups could not
 * become co-resident - or an XCD took no workgroups).  In that case every output row of the affected call is filled
 * with NaN.  The caller zeroes the word, runs any number of lc_lstm_* calls on the same workspace, and reads it at its
 * next synchronisation point (lc_optimizer_step can take it as `guard` so that a failed step leaves the parameters
 * untouched); on failure it re-runs the step with LC_LSTM_PERSISTENT=0.  The persistent schedule is only chosen on a
 * device that reports gfx950 with 256 CUs in 8 XCCs (SPX); anything else runs the launch train.
 * Environment (read per call; for tests): LC_LSTM_PERSISTENT=0 forces the launch train, LC_LSTM_SPIN_LIMIT=<n> bounds
 * every wait to n polls (default 2^21). */
#define LC_LSTM_STATUS_OFFSET 64
size_t lc_lstm_fwd_workspace_bytes(int B, int N, int ndir);
int lc_lstm_fwd(const lc_lstm_fwd_dir_t *dirs /* host array */, int ndir, const int *seq_len, int T, int B,
                int N, float forget_bias, void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* BPTT of lc_lstm_fwd.
 *   gates [T,B,4N] in: activated gates; out: dz (gradient w.r.t. the pre-activations)
 *   RT    [4N,N]   transpose of R
 *   dh    [T,B,N]  gradient w.r.t. m'_t coming from the layer output
 *   dpeep [3,N]    += gradients of (w_f, w_i, w_o); may be NULL
 *   dbias [4N]     += column sums of dz = gradient of the LSTM bias (same column layout as gates); may be NULL */
typedef struct {
    float *gates;
    const float *RT;
    const float *w_f, *w_i, *w_o;
    const float *cs;
    const float *dh;
    float *dpeep;
    float *dbias;
    int reverse;
    uint16_t *dz_bf16;   /* lc_lstm_bwd_bf16 only, may be NULL: [T,B,4N] bf16 (round-to-nearest-even) copy of dz, written in
                          * the same pass (the operand of dX = dz.Kx^T) */
    int shadow_only;     /* lc_lstm_bwd_bf16 with dz_bf16: non-zero = the caller reads dz only through dz_bf16 (every product of
                          * a c5 backward does); `gates` is then UNSPECIFIED after the call.  dpeep / dbias are exact as always. */
} lc_lstm_bwd_dir_t;
size_t lc_lstm_bwd_workspace_bytes(int B, int N, int ndir);
int lc_lstm_bwd(const lc_lstm_bwd_dir_t *dirs /* host array */, int ndir, const int *seq_len, int T, int B,
                int N, void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* bf16-operand variants (BASELINE.json configs[4]): identical contract, except that the two operands of the
 * step GEMM - the recurrent state m'_{t-1} (resp. dz_{t'}) and R (resp. R^T) - are rounded to bf16
 * (round-to-nearest-even) and multiplied by v_mfma_f32_16x16x32_bf16 with float32 accumulation.  Gates, cell
 * state, saved activations and every output stay float32.  Requires num_neurons % 32 == 0. */
int lc_lstm_fwd_bf16(const lc_lstm_fwd_dir_t *dirs /* host array */, int ndir, const int *seq_len, int T, int B,
                     int N, float forget_bias, void *workspace, size_t workspace_bytes, lc_stream_t stream);
int lc_lstm_bwd_bf16(const lc_lstm_bwd_dir_t *dirs /* host array */, int ndir, const int *seq_len, int T, int B,
                     int N, void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* Split-operand variants (config key compute_dtype = bf16x3): identical contract and fp32-grade results - the step product
 * m'_{t-1} . R (BPTT: dz_{t'} . R^T) is computed as in lc_gemm_bf16x3_nt: both fp32 operands split exactly into three bf16
 * terms (the forward state by the consumer, from the same tagged fp32 exchange fragments the fp32 kernels use; dz by its
 * producer; R once per call), the six term pairs of weight >= 2^-16 accumulated in fp32 on v_mfma_f32_16x16x32_bf16 (error
 * bound above).  Gates, cell state, saved activations and every output are the fp32 kernels'.  Split-operand kernels exist
 * for the XCD-pair schedule at num_neurons 768 / 1024 (schedule 6) and for the single-XCD schedule at num_neurons 64 .. 512
 * in steps of 64 (schedule 7), both passes each; the BPTT's exchange carries producer-split bf16 pieces, and its workspace
 * is the larger one lc_lstm_bwd_workspace_bytes already reports.  Every other shape - and the launch-train fall-back of a
 * failed persistent launch - runs the fp32 kernels of lc_lstm_fwd / lc_lstm_bwd (the same arithmetic in another summation order).
 * lc_lstm_bwd_x3 reads dirs[i].dz_bf16 (may be NULL) as the x3 SHADOW of dz - [T * B, 12 N] bf16 in the lc_split_bf16x3 layout,
 * the operand lc_gemm_bf16x3_nt / _tn read for dX / dKx / dR: the split-operand kernels' producers, which split dz for the
 * exchange anyway, write it (bit 18 of the schedule word); every other schedule gets lc_split_bf16x3 behind the recurrence. */
int lc_lstm_fwd_x3(const lc_lstm_fwd_dir_t *dirs /* host array */, int ndir, const int *seq_len, int T, int B,
                   int N, float forget_bias, void *workspace, size_t workspace_bytes, lc_stream_t stream);
int lc_lstm_bwd_x3(const lc_lstm_bwd_dir_t *dirs /* host array */, int ndir, const int *seq_len, int T, int B,
                   int N, void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* DropoutWrapper(output_keep_prob) on a layer output (bilstm.py:128,149):
 *   y[r,p] (+)= x[r,p] * Bernoulli(keep)/keep, the mask being a counter-based hash of
 *   (seed, stream_id, r*P+p) - regenerated, never stored.  x == y (in place) is allowed. */
int lc_dropout_scale(const float *x, int rows, int P, int ldx, float keep, uint32_t seed,
                     uint32_t stream_id, float *y, int ldy, int accumulate, lc_stream_t stream);
/* The same pass also writing the bf16 (round-to-nearest-even) copy of the result, y16 [rows, P] with row pitch ld16:
 * the operand shadow the next bf16 product reads (compute_dtype = bf16), without a separate lc_cast_bf16 pass over the
 * tensor.  P, ldx, ldy, ld16 multiples of 4; x / y 16-byte aligned, y16 8-byte aligned. */
int lc_dropout_scale_bf16(const float *x, int rows, int P, int ldx, float keep, uint32_t seed, uint32_t stream_id,
                          float *y, int ldy, int accumulate, uint16_t *y16, int ld16, lc_stream_t stream);

/* ------------------------------------------------------------------ MoE head ---------------- */
/* create_moe — nnet/moe.py:29-72, fused: logits[r,v] = sum_e softmax_E(a)[r,e] * tau*tanh(q[r,e*V+v]),
 * a = h.Wp+bp [R,E], q = h.W+b [R,E*V] (both produced by lc_gemm_f32). */
/* q is overwritten with tanh(q) (fwd) and then with dq (bwd); pi [R,E] keeps the softmax; da [R,E]. */
int lc_moe_combine_fwd(const float *a, float *q, int R, int E, int V, float tau, float keep,
                       uint32_t seed, float *logits, float *pi, lc_stream_t stream);
int lc_moe_combine_bwd(const float *pi, float *q, const float *dlogits, int R, int E, int V,
                       float tau, float keep, uint32_t seed, float *da, lc_stream_t stream);

/* ------------------------------------------------------------------ optimizer --------------- */
/* L2 (1e-5 * theta on the first n_decay elements) + global-norm clip + optimizer update over ONE flat
 * parameter buffer — nnet/graph.py:183-200.  optimizer: 0 sgd, 1 momentum(0.9),
 * 2 adam(0.9,0.999,1e-8, TF epsilon placement).  state: [n] (momentum) or [2n] (adam m|v).
 * norm_out: device float[2] = {global norm, clip scale}. */
/* guard: NULL, or a device int; when *guard != 0 at execution time the call leaves params and state untouched
 * (norm_out is still written) - see LC_LSTM_STATUS_OFFSET. */
int lc_optimizer_step(float *params, float *grads, size_t n, size_t n_decay, float l2,
                      float clip_norm, int optimizer, float lr, int step, float *state,
                      float *norm_out, const int *guard, void *workspace, size_t workspace_bytes,
                      lc_stream_t stream);
size_t lc_optimizer_workspace_bytes(size_t n);

/* column sums: out[N] (+)= sum_rows x[rows,N]  (bias gradients).  Deterministic: row slabs are summed into the
 * workspace (lc_colsum_workspace_bytes) and folded in a fixed order.  The workspace is REQUIRED: at least
 * N * sizeof(float) bytes (LC_EINVAL otherwise); one smaller than lc_colsum_workspace_bytes(N) selects a single slab
 * (same result for the same call, slower). */
size_t lc_colsum_workspace_bytes(int N);
int lc_colsum(const float *x, int rows, int N, int ldx, float *out, int accumulate, void *workspace,
              size_t workspace_bytes, lc_stream_t stream);
/* out[cols,rows] = in[rows,cols]^T */
int lc_transpose(const float *in, int rows, int cols, float *out, lc_stream_t stream);

/* KL label-smoothing regulariser of nnet/bilstm.py:255-269 over ALL rows (padded frames included):
 *   *loss_acc += weight * sum p*(log p - log q)   (device double, caller zeroes it);  q = uniform if log_q NULL
 *   dlogits  += its gradient (may be NULL). */
int lc_label_smoothing(const float *logits, int rows, int V, const float *log_q, float weight,
                       double *loss_acc, float *dlogits, lc_stream_t stream);

/* Softmax posteriors for nnet-forward: out = softmax(smooth*logits) or its log, minus prior
 * (nnet/graph.py:236, bin/nnet-forward.py:87-91). prior may be NULL. */
int lc_posteriors(const float *logits, int rows, int V, float smooth, int apply_softmax,
                  int apply_log, const float *log_prior, float *out, lc_stream_t stream);

/* ------------------------------------------------------------------ batch normalisation ----- */
/* tf.layers.batch_normalization as create_logits_lstm uses it (nnet/lstm.py:271-294; rank-3 input => TF's
 * non-fused path): per-column moments over ALL rows of x[rows, C] (rows = T*B, padded frames included),
 * population variance; y = (x - mean) * rsqrt(var + eps) * gamma + beta (eps = 1e-3 in the reference).
 *   lc_bn_moments        batch mean / variance (training)            workspace: lc_bn_workspace_bytes(C)
 *   lc_bn_apply          normalise with the given mean / var (batch moments, or the moving averages at inference)
 *   lc_bn_bwd            dx, dgamma, dbeta (overwritten); training != 0: gradient through the batch moments
 *   lc_bn_update_moving  assign_moving_average, v -= (v - batch) * (1 - momentum), the UPDATE_OPS of
 *                        nnet/graph.py:194-196 (momentum = 0.99).  TensorFlow's arithmetic bit for bit: the decay is
 *                        1 - momentum taken in double and THEN rounded to float (0.01f; 1.0f - 0.99f is 0.00999999f), the
 *                        product and the difference are rounded separately
 * dx may alias dy. */
size_t lc_bn_workspace_bytes(int C);
int lc_bn_moments(const float *x, int rows, int C, int ldx, float *mean, float *var, void *workspace,
                  size_t workspace_bytes, lc_stream_t stream);
int lc_bn_apply(const float *x, int rows, int C, int ldx, const float *mean, const float *var,
                const float *gamma, const float *beta, float eps, float *y, int ldy, lc_stream_t stream);
int lc_bn_bwd(const float *x, const float *dy, int rows, int C, int ldx, int lddy, const float *mean,
              const float *var, const float *gamma, float eps, int training, float *dx, int lddx,
              float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, lc_stream_t stream);
int lc_bn_update_moving(float *moving_mean, float *moving_var, const float *mean, const float *var, int C,
                        double momentum, lc_stream_t stream);
/* dynamic_rnn's zero output beyond sequence_length, re-applied to a time-major x[T*B, C] whose padded rows are no
 * longer zero (a ResidualWrapper input that went through batch normalisation): x[t*B+b, :] = 0 for t >= seq_len[b]. */
int lc_length_mask(float *x, int T, int B, int C, int ldx, const int *seq_len, lc_stream_t stream);

/* ------------------------------------------------------------------ packed frames ----------- */
/* A ragged batch's live frames as a dense matrix (nnet/frames.py: FrameMap; no reference counterpart): the products that
 * read a layer's INPUT run on `Mp` packed rows instead of T * B padded ones.  Row maps are device int32, -1 = no source row.
 *   lc_pack_rows    out[r, :] = rows[r]    >= 0 ? x[rows[r], :]    : 0   for r < Mp           (padded -> packed)
 *   lc_unpack_rows  out[q, :] = inverse[q] >= 0 ? x[inverse[q], :] : 0   for q < rows = T * B (packed -> padded)
 * Every output row is written exactly once (no memset needed, deterministic); zero rows are +0.0.  ldx / ldo: row pitches in
 * floats (column windows of wider buffers are fine).  C % 4 == 0 with 16-byte aligned rows takes 16-byte accesses, anything
 * else a scalar path.  A map entry must name a row of x: the caller's contract, nothing here can check it. */
int lc_pack_rows(const float *x, int ldx, const int *rows, int Mp, int C, float *out, int ldo, lc_stream_t stream);
int lc_unpack_rows(const float *x, int ldx, const int *inverse, int rows, int C, float *out, int ldo, lc_stream_t stream);

/* ------------------------------------------------------------------ chunked batch ---------- */
/* The layout passes of the latency-controlled BiLSTM (Zhang et al. 2016; Xue & Yan 2017; no reference counterpart; DESIGN.md
 * 3.13): the backward direction of a layer restarts from a zero state in every chunk of `chunk` frames, after `lookahead`
 * warm-up frames.  It runs as the ordinary reverse recurrence (lc_lstm_fwd / lc_lstm_bwd, reverse = 1) on a re-laid-out batch:
 *   nC = ceil(T / chunk) chunks, Tc = min(chunk + lookahead, T) frames each, Bc = nC * B rows;
 *   the chunked layout is time-major [Tc, Bc, C], chunk row r = c * B + b holds frames [c * chunk, c * chunk + Tc) of
 *   utterance b, and its length is clamp(seq_len[b] - c * chunk, 0, Tc).
 *   lc_chunk_gather  (padded -> chunked)  with t = c * chunk + tau:
 *                    out[(tau * Bc + c * B + b) * ldo + k] = x[(t * B + b) * ldx + k]  if t < T and (!zero_lookahead or
 *                    tau < chunk), else +0.  zero_lookahead = 0 serves zx; 1 serves dh (the outputs of lookahead frames are
 *                    discarded, so their upstream gradient is zero).
 *   lc_chunk_fold    (chunked -> padded)
 *                    sum_copies = 0: out[t, b, :] = the copy of the frame's own chunk, c = t / chunk, tau = t % chunk, bit
 *                    for bit (serves hs);
 *                    sum_copies != 0: out[t, b, :] = the float32 sum over every chunk c with c * chunk <= t < c * chunk + Tc,
 *                    in ascending c, the first term initialising the sum (no 0 + ...) (serves dz: zx[t] is shared by every
 *                    chunk copy of frame t);
 *                    seq_len (device [B] int32) non-NULL: a copy whose tau is at or beyond its chunk row's length is skipped
 *                    and rows with t >= seq_len[b] are +0 - the result does not depend on what a recurrence left in dead
 *                    frames.
 * Every element of out is written on every call (no memset needed).  A pure function of its arguments (no atomics): the same
 * call gives the same bits.  Elements are indexed in 64 bits.  ldx / ldc / ldo: row pitches in floats (column windows of wider
 * buffers are fine).  16-byte accesses when C and both pitches are multiples of 4 and both bases 16-byte aligned, a scalar
 * path otherwise.
 * LC_EINVAL, with nothing launched and no output touched: T, B, C <= 0; chunk <= 0; lookahead < 0; a NULL x / xc / out; a pitch
 * below C. */
int lc_chunk_gather(const float *x, int ldx, int T, int B, int C, int chunk, int lookahead, int zero_lookahead, float *out,
                    int ldo, lc_stream_t stream);
int lc_chunk_fold(const float *xc, int ldc, int T, int B, int C, int chunk, int lookahead, int sum_copies,
                  const int *seq_len /* or NULL */, float *out, int ldo, lc_stream_t stream);

/* ------------------------------------------------------------------ row convolution --------- */
/* Row convolution (lookahead convolution; Amodei et al. 2016, "Deep Speech 2"; no reference counterpart): one
 * depthwise filter over the next tau frames of the uni-LSTM's top layer, tau frames of lookahead for (tau + 1) * C parameters.
 * x, y, dy, dx are time-major [T * B, C] with row pitches ldx / ldy / lddy / lddx in floats (column windows of wider buffers
 * are fine); w and dw are dense [tau + 1, C]; seq_len is a device [B] int32 and is REQUIRED.  With
 * len_b = clamp(seq_len[b], 0, T) and live(t, b) = t < len_b:
 *   lc_row_conv_fwd   y[t, b, c]  = sum over j = 0 .. tau with live(t + j, b) of w[j, c] * x[t + j, b, c]   if live(t, b), else +0
 *   lc_row_conv_bwd   dx[t, b, c] = sum over j = 0 .. min(tau, t) of w[j, c] * dy[t - j, b, c]               if live(t, b), else +0
 *                     dw[j, c]    = sum over b and over t with live(t + j, b) of dy[t, b, c] * x[t + j, b, c]  (overwritten, not
 *                                   accumulated)
 *   - Dead rows are never read: a frame at or past len_b contributes nothing whatever it holds (NaN included), so the result
 *     does not depend on the padding or on what else is in the batch.
 *   - Full writes: every element of y, dx and dw is written on every successful call (no memset needed), and nothing outside
 *     the [T * B, C] windows (the [tau + 1, C] block of dw) is touched.
 *   - Summation order of y and dx: ascending j, the first term initialising the sum (no 0 + ...); FMA contraction is allowed.
 *     A kernel that is 1 in row j0 and 0 elsewhere therefore copies finite inputs exactly.
 *   - Determinism: no atomics.  dw sums row slabs into the workspace and folds them in a fixed order, like lc_colsum; its
 *     summation order is otherwise unspecified.  The same call gives the same bits.
 *   - Pointers: dx or dw may be NULL, not both; x may be NULL when dw is.  x and y must not overlap, nor dx and dy (equal
 *     pointers included); two disjoint column windows of one buffer do not overlap.
 *   - Elements are indexed in 64 bits.  16-byte accesses when C and the pitches are multiples of 4 and the bases (w and the
 *     workspace included) 16-byte aligned, a scalar path otherwise.
 * LC_EINVAL, with nothing launched and no output touched: T, B, C <= 0; tau < 0 or tau > 32 (a design cap: the weights of a
 * column group live in LDS); a NULL required pointer; a pitch below C; the overlaps above.  LC_EWORKSPACE, likewise: a non-NULL
 * dw with a workspace below lc_row_conv_workspace_bytes (0 for a bad shape). */
size_t lc_row_conv_workspace_bytes(int T, int B, int C, int tau);
int lc_row_conv_fwd(const float *x, int ldx, const float *w, int T, int B, int C, int tau, const int *seq_len, float *y, int ldy,
                    lc_stream_t stream);
int lc_row_conv_bwd(const float *x, int ldx, const float *dy, int lddy, const float *w, int T, int B, int C, int tau,
                    const int *seq_len, float *dx /* or NULL */, int lddx, float *dw /* or NULL */, void *workspace,
                    size_t workspace_bytes, lc_stream_t stream);

/* ------------------------------------------------------------------ time reduction ---------- */
/* The layout passes of the pyramidal BiLSTM (Chan et al. 2016, "Listen, Attend and Spell"; no reference counterpart; DESIGN.md
 * 3.17): r consecutive frames of a layer's output become one frame, r times as wide, of the next layer's input, which then
 * runs on To = ceil(T / r) frames.  x and dx are time-major [T * B, C] with row pitches ldx / lddx in floats, y and dy are
 * time-major [To * B, r * C] with row pitches ldy / lddy (column windows of wider buffers are fine); seq_len is a device [B]
 * int32 and is REQUIRED.  With len_b = clamp(seq_len[b], 0, T):
 *   lc_time_reduce_fwd   y[to, b, j * C + c] = x[r * to + j, b, c]            if r * to + j < len_b, else +0, for j < r
 *   lc_time_reduce_bwd   dx[t, b, c]         = dy[t / r, b, (t % r) * C + c]  if t < len_b, else +0
 *   - Full writes: every element of the output window ([To * B, r * C] of y, [T * B, C] of dx) is written on every successful
 *     call (no memset needed), and nothing outside the window is touched.  A last group that T or the utterance's end cuts
 *     short is filled with +0.
 *   - Copies are bit exact.  A dead source frame is never read: a NaN in a frame at or past len_b, or in a pad column beyond a
 *     window, has no effect.
 *   - A pure function of its arguments (no atomics): the same call gives the same bits.
 *   - Elements are indexed in 64 bits.  16-byte accesses when C and both pitches are multiples of 4 and both bases 16-byte
 *     aligned, a scalar path otherwise.
 * LC_EINVAL, with nothing launched and no output touched: T, B, C <= 0; r < 2 or r > 4; a NULL pointer; ldx / lddx below C or
 * ldy / lddy below r * C; input and output windows whose byte ranges overlap. */
int lc_time_reduce_fwd(const float *x, int ldx, int T, int B, int C, int r, const int *seq_len, float *y, int ldy,
                       lc_stream_t stream);
int lc_time_reduce_bwd(const float *dy, int lddy, int T, int B, int C, int r, const int *seq_len, float *dx, int lddx,
                       lc_stream_t stream);

/* ------------------------------------------------------------------ layer normalisation ----- */
/* Layer normalisation of a layer's output (Ba et al. 2016; no reference counterpart), with the DropoutWrapper
 * mask behind it.  x, y, dy, dx are time-major [T * B, C] with row pitches ldx / ldy / lddy / lddx in floats (column windows of
 * wider buffers are fine); gamma, beta, dgamma, dbeta are dense [C]; seq_len is a device [B] int32 and is REQUIRED.  With
 * len_b = clamp(seq_len[b], 0, T), live(t, b) = t < len_b, m = mean_c x, v = mean_c (x - m)^2 (biased), rstd = 1 / sqrt(v + eps),
 * xh = (x - m) * rstd, row r = t * B + b, and mask[r, c] = the DropoutWrapper factor (1 / keep or 0) of stream
 * stream0 + c / drop_width at index r * drop_width + c % drop_width - what lc_dropout_scale gives on the [T * B, drop_width]
 * column window c / drop_width with stream_id = stream0 + c / drop_width -, 1 when keep == 1:
 *   lc_layer_norm_fwd   y[r, c]   = mask[r, c] * (gamma[c] * xh[r, c] + beta[c])                        if live, else +0
 *   lc_layer_norm_bwd   with g = mask * dy, a = gamma * g:
 *                       dx[r, c]  = rstd * (a[r, c] - mean_c a - xh[r, c] * mean_c (a * xh))            if live, else +0
 *                       dgamma[c] = sum over live rows of g * xh,   dbeta[c] = sum over live rows of g  (overwritten)
 *   - One streaming pass each: a row is read once into registers and written once; the backward recomputes m and rstd from x,
 *     so no statistics are kept between the passes.  The variance is the centred two-pass form, not E[x^2] - m^2.
 *   - Dead rows are never read (NaN included) and written +0; every element of y, dx, dgamma and dbeta is written on every
 *     successful call, and nothing outside the windows is touched.
 *   - With keep < 1, y equals lc_dropout_scale applied to the keep == 1 result, bit for bit.
 *   - Determinism: no atomics.  Each workgroup of the backward walks a fixed, contiguous share of the rows and leaves one
 *     [2, C] partial in the workspace; a second kernel adds the partials in a fixed order.  The same call gives the same bits.
 *   - Pointers: dx may be NULL; dgamma and dbeta are both NULL or both not; not all three.  The workspace is needed for the
 *     parameter gradients only.  dx == dy with lddx == lddy is allowed (in place); any other overlap of y with x, of dx with x
 *     or of dx with dy is refused.
 *   - Elements are indexed in 64 bits.  16-byte accesses when C and the pitches are multiples of 4 and the bases (gamma and beta
 *     included) 16-byte aligned, a scalar path otherwise.
 * LC_EINVAL, with nothing launched and no output touched: T, B, C <= 0 or C > 8192 (a design cap: a row lives in one wave's
 * registers); a NULL required pointer; one of dgamma / dbeta alone; a pitch below C; eps <= 0; keep outside (0, 1]; drop_width
 * < 1 or not a divisor of C; the overlaps above; a non-NULL dgamma with a workspace below lc_layer_norm_workspace_bytes (0 for
 * a bad shape). */
size_t lc_layer_norm_workspace_bytes(int T, int B, int C);
int lc_layer_norm_fwd(const float *x, int ldx, const float *gamma, const float *beta, int T, int B, int C, float eps,
                      const int *seq_len, float keep, uint32_t seed, uint32_t stream0, int drop_width,
                      float *y, int ldy, lc_stream_t stream);
int lc_layer_norm_bwd(const float *x, int ldx, const float *dy, int lddy, const float *gamma, int T, int B, int C, float eps,
                      const int *seq_len, float keep, uint32_t seed, uint32_t stream0, int drop_width,
                      float *dx /* or NULL */, int lddx, float *dgamma, float *dbeta /* both or neither; overwritten */,
                      void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* ------------------------------------------------------------------ convolutional front-end - */
/* One layer of the 2-D convolutional front-end between the features and the first LSTM layer (Deep Speech 2, VGG-BLSTM; no
 * reference counterpart): kernel 3 (time) x 3 (frequency), time stride 1, frequency stride 2, zero padding 1 on
 * every side, bias and ReLU fused - torch.nn.functional.conv2d(padding=1, stride=(1, 2)) + relu with the dead-frame rule.
 * x / dx are time-major [T * B, Cin * F] with row pitches ldx / lddx in floats; with x_group_major != 0 column ci * F + f (the
 * loader's layout: statics, deltas and delta-deltas as blocks of F bins), otherwise column f * Cin + ci (what a previous
 * layer writes).  y / dy are [T * B, Fo * Cout], column fo * Cout + co, Fo = ceil(F / 2), pitches ldy / lddy.  w / dw are dense
 * [3, 3, Cin, Cout] (time tap i, bin tap j, in, out), bias / dbias dense [Cout]; seq_len is a device [B] int32 and is REQUIRED.
 * With len_b = clamp(seq_len[b], 0, T), live(t, b) = t < len_b, xz = x on live frames and bins 0 .. F - 1 and 0 everywhere else
 * (those elements are never read), and g = dy where y > 0, else 0:
 *   lc_conv_fwd   y[t,b,fo,co]   = relu(bias[co] + sum_{i,j,ci} w[i,j,ci,co] * xz[t+i-1, b, 2fo+j-1, ci])       if live, else +0
 *   lc_conv_bwd   dx[t,b,f,ci]   = sum over (i, j, fo, co) with live(t-i+1, b) and 2fo+j-1 == f of
 *                                  w[i,j,ci,co] * g[t-i+1,b,fo,co]                                             if live, else +0
 *                 dw[i,j,ci,co]  = sum over b, live t, fo of g[t,b,fo,co] * xz[t+i-1,b,2fo+j-1,ci]
 *                 dbias[co]      = sum over b, live t, fo of g[t,b,fo,co]                                      (both overwritten)
 *   - Three direct convolutions on fp32 FMAs over LDS tiles: a workgroup stages a segment of frames with one halo row on each
 *     side, so a row is fetched once per segment and not once per tap, and 8 channels of the reduction at a time.
 *   - Dead rows of x, y and dy are never read (NaN included) and written +0; neighbouring utterances never leak into each other
 *     (rows t - 1 and t + 1 are the SAME utterance's); every element of every non-NULL output is written on every successful
 *     call, and nothing outside the windows is touched.
 *   - Determinism: no atomics.  Each workgroup of the weight gradient walks a fixed, contiguous share of the tiles and leaves
 *     one [9 Cin Cout + Cout] partial in the workspace; a second kernel adds the partials in a fixed order.  The same call
 *     gives the same bits.
 *   - Pointers: dx may be NULL (the first layer); dw and dbias are both NULL or both not; not all three.  x is needed for dw
 *     only, the workspace too.
 *   - Elements are indexed in 64 bits.  y (and a channel-minor dx with Cin a multiple of 4) are written with 16-byte stores,
 *     and the weight gradient reads y and dy with 16-byte loads, when the pitches are multiples of 4 floats and the bases
 *     16-byte aligned; the scalar path otherwise, and for every other access.
 * LC_EINVAL, with nothing launched and no output touched: T, B, F, Cin, Cout <= 0; Cin > 64, Cout > 64, Cout not a multiple of
 * 8 or F > 512 (design caps: a workgroup's weight chunk and partial live in LDS, a thread owns 4 output channels); a NULL
 * required pointer; one of dw / dbias alone; all three gradient outputs NULL; a pitch below its row; an output window that
 * overlaps an input window or another output.  LC_EWORKSPACE: a non-NULL dw with a workspace below lc_conv_workspace_bytes
 * (0 for a bad shape). */
size_t lc_conv_workspace_bytes(int T, int B, int F, int Cin, int Cout);
int lc_conv_fwd(const float *x, int ldx, int x_group_major, const float *w, const float *bias,
                int T, int B, int F, int Cin, int Cout, const int *seq_len, float *y, int ldy, lc_stream_t stream);
int lc_conv_bwd(const float *x, int ldx, int x_group_major, const float *y, int ldy, const float *dy, int lddy,
                const float *w, int T, int B, int F, int Cin, int Cout, const int *seq_len,
                float *dx /* or NULL */, int lddx, float *dw, float *dbias /* both or neither; overwritten */,
                void *workspace, size_t workspace_bytes, lc_stream_t stream);

/* ------------------------------------------------------------------ SpecAugment ------------- */
/* Time and frequency masking of the filterbank input (Park et al., 2019; no reference counterpart), on the spliced and
 * subsampled batch the loader uploads.  x and out are time-major [T * B, D] with row pitches ldx / ldo (floats); out == x (in
 * place) is allowed.
 * Layout: with s = max(subsample, 1) and l, r the contexts, column c of row (t, b) belongs to spliced block i = c / base_dim;
 * it shows raw frame u = clamp(t * s + i - l, 0, n - 1), n = seq_len[b] * s, and bin f = (c % base_dim) % freq_bins.
 *   - the utterance is treated as having exactly n raw frames: the loader drops the T_raw % s tail, and the true raw length
 *     does not reach the device;
 *   - this is exact whenever r <= s - 1, which covers the recipes;
 *   - otherwise the last rows' right-context copies of frames past n - 1 count as frame n - 1.
 * Draws (all integer arithmetic): hash(k) = the 32-bit value lc_dropout_factor forms before its float conversion, for
 * (seed, stream id 0x53504543, 64-bit index b * 32 + k); ranged(v, m) = ((uint64_t)v * m) >> 32.
 *   time mask j < time_masks:  W = min(time_width, n * time_percent / 100) (64-bit integer division),
 *                              w = ranged(hash(2j), W + 1), t0 = ranged(hash(2j + 1), n - w + 1): raw frames [t0, t0 + w)
 *   freq mask j < freq_masks:  w = ranged(hash(16 + 2j), freq_width + 1), f0 = ranged(hash(17 + 2j), freq_bins - w + 1):
 *                              bins [f0, f0 + w) of every feature group and every spliced block
 * Masks are drawn per utterance, may overlap, and may have width 0.
 * Output: for t < seq_len[b], out = fill where a time mask holds u or a frequency mask holds f, out = x bit for bit elsewhere;
 * rows with t >= seq_len[b] are copied unchanged; every element of out is written on every call.  plan (device [B,16,2] int32,
 * or NULL) receives (start, width) per mask: rows 0-7 the time masks, rows 8-15 the frequency masks, unused rows (0, 0).
 * A pure function of its arguments (no atomics): the same call gives the same bits.
 * LC_EINVAL, with nothing launched and no output touched: T, B, D <= 0; a NULL x / seq_len / cfg / out; a pitch below D; a mask
 * count outside 0..8; a negative width; time_percent outside 0..100; freq_bins <= 0; base_dim % freq_bins != 0; freq_width >
 * freq_bins; D != base_dim * (1 + l + r); negative contexts or subsample; a fill that is not finite.
 * 16-byte accesses when D and both pitches are multiples of 4 and both bases 16-byte aligned, a scalar path otherwise. */
typedef struct lc_spec_augment {
    int time_masks, time_width, time_percent;   /* 0..8 masks; width cap in RAW frames; cap in percent of the utterance, 0..100 */
    int freq_masks, freq_width, freq_bins;      /* 0..8 masks; width cap in bins; F = bins per feature group */
    int base_dim, left_context, right_context, subsample;   /* the loader's layout: D = base_dim * (1 + l + r) */
    float fill;                                 /* value written into masked elements (finite) */
} lc_spec_augment_t;
int lc_spec_augment(const float *x, int T, int B, int D, int ldx, const int *seq_len, const lc_spec_augment_t *cfg /* host */,
                    uint32_t seed, float *out, int ldo, int *plan /* device [B,16,2] or NULL */, lc_stream_t stream);

/* ------------------------------------------------------------------ development hook -------- */
/* Not part of the product surface: when set to a device buffer of [T][4 waves][8] 64-bit words, one workgroup of
 * the forward step kernel stores s_memtime stamps of its phases there (tools/stamp_probe.py); NULL switches it off. */
void lc_debug_set_lstm_stamps(unsigned long long *buf);
/* Which schedule the calling thread's last lc_lstm_fwd* / lc_lstm_bwd* call took (tests assert it):
 *   bits 0-7   1 = persistent float32, 2 = persistent bf16, 3 = two-stream launch train, 4 = launch train,
 *              5 = persistent float32 over XCD pairs (num_neurons 640 / 768 / 896 / 1024),
 *              6 = split-operand (bf16x3) recurrence over XCD pairs (num_neurons 768 / 1024), 7 = split-operand, one XCD
 *              per (direction, row group) (num_neurons 64 .. 512 in steps of 64)
 *   bits 8-15  row tiles of 16 per workgroup (launch train), bit 16 = bf16 operands, bit 17 = backward,
 *   bit 18 = the x3 shadow of dz was written by the BPTT kernel itself (lc_lstm_bwd_x3). */
int lc_debug_last_lstm_schedule(void);
/* Same kind of hook for the CTC scan: device buffer of [2 phases][5 waves][512 iterations][8] 64-bit s_memtime stamps
 * of workgroup 0 (tools/ctc_stamps.py); NULL switches it off. */
void lc_debug_set_ctc_stamps(unsigned long long *buf);
/* Which kernels the calling thread's last SUCCESSFUL lc_ctc_loss call dispatched (tests assert it); 0 before the first:
 *   bits 0-3    1 = two launches of the meet-in-the-middle kernel, 2 = three kernels (row statistics, scan, gradient)
 *   bits 4-9    PPL, lattice positions per lane of the scan      bits 10-13  NW, scan waves per direction
 *   bits 14-17  KG, classes per lane of the frame waves (3: V <= 48, 5: V <= 80, 8: V <= 128; 0 on the three-kernel path)
 *   bit 18      the frame statistics were taken in phase 2 ("ctc_lse2")
 *   bits 19-25  lanes per frame of the row-statistics kernel (three-kernel path: 16 for V <= 32, else 64). */
int lc_debug_last_ctc_path(void);
/* Which of lc_ctc_align's three launches run (process-wide; tools/align_probe.py times them one by one on a workspace a
 * full call has filled): bit 0 = per-frame log-sum-exp, bit 1 = forward sweep, bit 2 = backtrace.  Default 7. */
void lc_debug_ctc_align_phases(int mask);
/* A FOREIGN resident kernel for tests: `blocks` workgroups of 256 threads that stay resident for `microseconds` of wall
 * clock, hold `lds_bytes` of LDS each and do nothing else - what a collective's kernel waiting for a slower peer looks like
 * to the next persistent recurrence (one workgroup with >= 84 KB of LDS per CU on every CU of an XCD: with lds_bytes >= 80 KB
 * the two cannot share a CU).  tests/test_gpu_coresidency.py rehearses that hazard with it. */
int lc_debug_spin(int blocks, int microseconds, int lds_bytes, lc_stream_t stream);
/* The whole-round rule of the 256 x 256 product kernels (HOST arithmetic, no GPU needed): of `row_tiles` x `col_tiles` tiles
 * of an unsplit product, how many row tiles the big kernel takes so that its rounds of `cus` workgroups (0 = the current
 * device's CU count, 256 without a device) are whole; the rows behind them run on the 128 x 128 kernel.  tests/test_host.py. */
int lc_debug_gemm_whole_round_row_tiles(int row_tiles, int col_tiles, int cus);

/* ------------------------------------------------------------------ input path (HOST) ------- */
/* TFRecord + tf.train.SequenceExample decoding without TensorFlow: what tf.data.TFRecordDataset(...).map(_parse,
 * num_parallel_calls) does per utterance in nnet/tfrecord.py:94-125, with _splice (28-40) and _subsample (43-51) fused
 * into the copy.  HOST functions on HOST buffers, no GPU involved, thread-safe and re-entrant: the loader calls them from
 * `--num-parallel-calls` worker threads (ctypes releases the GIL).  `file` is the whole .tfrecords file image; its FIRST
 * record is the utterance (the reference's converter writes one SequenceExample per file, tfrecord.py:128-156).
 *   lc_tfrecord_inspect: validates the framing - with verify_crc != 0 both masked CRC-32C words, as TF's reader does
 *     (a mismatch is LC_EINVAL "corrupted record") - and counts: frames and dim of feature list "nnet_input" (every frame
 *     must have the same number of floats), steps of "nnet_target".
 *   lc_tfrecord_decode: writes row j of the spliced / subsampled matrix to x + j * x_row_stride (floats), j < T',
 *     T' = subsample ? T / subsample : T, row width dim * (1 + left + right), edge frames replicated; and the labels
 *     (one int64 per step) to labels[].  x or labels may be NULL.  A row stride larger than the row width lets the caller
 *     decode straight into one utterance's rows of a padded TIME-MAJOR batch [T, B, D'] (stride B * D').
 *   lc_crc32c: plain (unmasked) CRC-32C (Castagnoli), hardware instruction when the CPU has it. */
typedef struct {
    int64_t num_frames;  /* T: features in "nnet_input" (before subsampling) */
    int32_t dim;         /* floats per frame (before splicing) */
    int32_t has_input, has_target;
    int64_t num_labels;  /* features in "nnet_target" */
} lc_seqex_info_t;
int lc_tfrecord_inspect(const void *file, size_t nbytes, int verify_crc, lc_seqex_info_t *info);
int lc_tfrecord_decode(const void *file, size_t nbytes, int dim, int left_context, int right_context, int subsample,
                       float *x, size_t x_row_stride, int64_t max_rows, int64_t *labels, int64_t max_labels);
uint32_t lc_crc32c(const void *data, size_t nbytes);
/* A whole padded batch in two calls, each fanned out over `nthreads` native threads (the tf.data map + padded_batch of
 * tfrecord.py:122-123 / pipeline.py:35-61).  lc_batch_open reads the n files, verifies their CRCs and reports raw frame
 * and label counts (num_labels[i] = -1 for a record without an "nnet_target" list: a caller whose tfrecords.scp says
 * has_label = 1 must treat that as an error, as tf.parse_single_sequence_example does for a missing feature list, tfrecord.py:
 * 94-105; dimension checked against expect_dim when > 0); a file with bytes behind its first record is refused; the caller sizes the batch; lc_batch_decode writes
 * utterance i's row j to x + i * utt_stride + j * row_stride (floats) - time-major [T,B,D']: utt_stride = D',
 * row_stride = B * D'; batch-major [B,T,D']: utt_stride = T * D', row_stride = D' - zero-fills its rows up to max_rows,
 * and writes its labels to labels + i * label_stride, padded with pad_label up to max_labels.  The first failing file
 * ends the call with its path in lc_last_error().  lc_batch_close frees the reader (always call it after a
 * successful open). */
typedef struct lc_batch_reader lc_batch_reader_t;
int lc_batch_open(const char *const *paths, int n, int verify_crc, int expect_dim, int nthreads,
                  lc_batch_reader_t **reader, int64_t *num_frames, int64_t *num_labels);
int lc_batch_decode(lc_batch_reader_t *reader, int left_context, int right_context, int subsample, float *x,
                    size_t utt_stride, size_t row_stride, int64_t max_rows, int64_t *labels, size_t label_stride,
                    int64_t max_labels, int64_t pad_label, int nthreads);
void lc_batch_close(lc_batch_reader_t *reader);

#ifdef __cplusplus
}
#endif
#endif
