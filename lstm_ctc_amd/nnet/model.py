"""The acoustic model: deep (Bi)LSTM-P stack + affine or high-rank (MoE) head, forward and backward.

Host-side mirror of mobvoi/lstm_ctc ``nnet/bilstm.py:25-273`` (``create_logits_blstm``),
``nnet/lstm.py:125-368`` (``create_logits_lstm``, intent) and ``nnet/moe.py:29-72`` (``create_moe``).
All arithmetic is done by ``liblstm_ctc_hip.so`` through :mod:`lstm_ctc_amd.ops`; this file only
owns buffers and sequencing.

MI355X-first design choices:

* activations are time-major ``[T*B, width]`` row-major matrices, so every batched op is one GEMM;
* ``x_t . Kx`` is hoisted over all T, the projection is folded into the recurrent weights
  (``R = proj . Kh``), so each time step is ONE dependent ``[B,N] x [N,4N]`` GEMM + gate math,
  both directions in the same call (``lc_lstm_fwd`` / ``lc_lstm_bwd``: one launch for both, or one chain per
  direction on two streams);
* ``tf.reverse_sequence`` never materialises: the reverse direction just walks t downwards;
* forward/backward layer outputs land in the two column halves of one ``[T*B, 2P]`` buffer;
* every LSTM ``kernel``/``bias`` lives permanently in the gate-interleaved column layout the step
  kernel wants; TF's ``[i|j|f|o]`` layout only exists at checkpoint I/O (:meth:`ParamStore.export_tf`);
* all parameters (and gradients, and optimizer slots) are single flat fp32 buffers: L2-decayed
  tensors first, the LSTM ``bias`` vectors (the only names containing "bias", nnet/graph.py:185) last - and behind them, with
  ``layer_norm``, the gains and offsets ``ln{i}/gamma``, ``ln{i}/beta``, undecayed by kind.  The convolutional front-end's
  ``conv{k}/kernel`` lie behind the LSTM layers' decayed tensors, its ``conv{k}/bias`` behind the LSTM biases.
"""
import math
import os

import numpy as np
import torch

from .. import ops


# variable scope of layer i's cell under tf.nn.dynamic_rnn(MultiRNNCell([CudnnCompatibleLSTMCell ...])) (nnet/lstm.py:73-96)
CUDNN_CELL = "rnn/multi_rnn_cell/cell_%d/cudnn_compatible_lstm_cell"


def gate_perm(N):
    """perm[c'] = c: interleaved column c' = (n//8)*32 + g*8 + n%8  <-  TF column c = g*N + n."""
    assert N % 8 == 0
    cp = np.arange(4 * N)
    blk, rem = cp // 32, cp % 32
    g, i = rem // 8, rem % 8
    return g * N + blk * 8 + i


class ParamStore:
    """Flat fp32 parameter / gradient buffers with named views (TF variable names)."""

    def __init__(self, cfg, device):
        self.cfg = cfg
        self.device = device
        self.blstm = cfg.get("nnet_type", "blstm") == "blstm"
        # 'cudnnlstm' (nnet/lstm.py:26-122): a MultiRNNCell of CudnnCompatibleLSTMCell(num_units) - plain LSTM cells: no
        # peepholes, no projection, forget bias 0, no dropout, no residual; the config's num_projects / use_peepholes are
        # read and logged there but never reach the cell
        self.cudnn = cfg.get("nnet_type") == "cudnnlstm"
        D = cfg["input_dim"] * (1 + (cfg.get("left_context") or 0) + (cfg.get("right_context") or 0))
        N, P, V = cfg["num_neurons"], cfg.get("num_projects"), cfg["num_targets"]
        if self.cudnn:
            if P and P != N:
                # lstm.py:99-102 reshapes the [.., num_neurons] cell output to [-1, num_projects]: anything but
                # num_projects == num_neurons scrambles frames there; refuse instead of reproducing that
                raise ValueError("cudnnlstm: num_projects (%d) must be absent or equal num_neurons (%d): the cell has no "
                                 "projection (nnet/lstm.py:74-76,99)" % (P, N))
            P = None
        self.D, self.N, self.P, self.V = D, N, (P or 0), V
        self.Pout = P if P else N
        # lstm.py:240 hard-codes True for 'lstm'; CudnnCompatibleLSTMCell has none
        self.peep = False if self.cudnn else (True if not self.blstm else bool(cfg.get("use_peepholes") or False))
        self.num_layers = cfg["num_layers"]
        self.E = (cfg.get("num_experts") or 0) if self.blstm else 0
        # pyramidal BiLSTM (extension keys time_reduce_layers / time_reduce_factor): a reduced layer reads r
        # frames of the layer below side by side - its kernels are r times as tall in their input part, nothing else moves
        self.time_reduce, self.time_reduce_factor = time_reduce_config(cfg)
        # convolutional front-end (extension keys conv_layers / conv_channels / conv_bins): layer 0 reads the
        # last conv layer's [F_n * Cc] columns where it read the D input columns - its kernel is that tall, nothing else moves
        self.conv = conv_config(cfg)
        self.D0 = self.conv[-1][3] * self.conv[-1][1] if self.conv else D
        D0 = self.D0
        specs = []       # (name, shape, kind)
        for i in range(self.num_layers):
            if self.blstm:
                I = D0 if i == 0 else (self.time_reduce_factor if i in self.time_reduce else 1) * 2 * self.Pout
                prefixes = ["fd%d/frnn%d" % (i, i), "bd%d/brnn%d" % (i, i)]       # bilstm.py:135,156,178,187
            elif self.cudnn:
                I = D0 if i == 0 else N
                prefixes = [CUDNN_CELL % i]                                        # lstm.py:73-88 (MultiRNNCell scopes)
            else:
                I = D0 if i == 0 else self.Pout
                prefixes = ["drnn%d/lstm_cell" % i]                                # lstm.py:279-287
            for pre in prefixes:
                specs.append((pre + "/kernel", (I + self.Pout, 4 * N), "lstm_kernel"))
                specs.append((pre + "/bias", (4 * N,), "lstm_bias"))
                if self.peep:
                    for nm in ("w_f_diag", "w_i_diag", "w_o_diag"):
                        specs.append((pre + "/" + nm, (N,), "peephole"))
                if P:
                    specs.append((pre + "/projection/kernel", (N, P), "proj"))
        # tf.layers.batch_normalization of the uni-LSTM (lstm.py:271-294): first-layer input + every layer output
        self.use_bn = bool(cfg.get("use_bn") or False) and not self.blstm and not self.cudnn
        self.bn_names = (["drnn_bn_0_0"] + ["drnn_bn%d" % i for i in range(self.num_layers)]) if self.use_bn else []
        self.aux_specs = []      # non-trainable variables (moving averages): saved/restored, never optimised
        for j, bn in enumerate(self.bn_names):
            C = D if j == 0 else self.Pout
            specs += [(bn + "/gamma", (C,), "bn_gamma"), (bn + "/beta", (C,), "bn_beta")]
            self.aux_specs += [(bn + "/moving_mean", (C,), 0.0), (bn + "/moving_variance", (C,), 1.0)]
        H = (2 if self.blstm else 1) * self.Pout
        self.H = H
        # row convolution (extension key row_conv_frames): one [tau + 1, H] filter between the top layer (its
        # batch norm) and the head - behind the layers' tensors, so that layer_grad_range and the data-parallel buckets keep
        # their ranges; no "bias" in the name: L2-decayed like every other kernel
        self.row_conv = row_conv_config(cfg)
        if self.row_conv:
            specs.append(("row_conv/kernel", (self.row_conv + 1, H), "row_conv"))
        # the front-end's layers: behind the LSTM layers' tensors too (layer_grad_range and the data-parallel buckets keep their
        # ranges; these gradients are the last to become ready and go out with GradientBuckets.finish()).  The kernels are
        # L2-decayed, the biases undecayed through the "bias" in their names
        for k, (Cin, Cc, _, _) in enumerate(self.conv):
            specs += [("conv%d/kernel" % k, (3, 3, Cin, Cc), "conv_kernel"), ("conv%d/bias" % k, (Cc,), "conv_bias")]
        # layer normalisation (extension key layer_norm): a gain and an offset per layer output.  Kept out of the
        # L2 decay by kind (a gain decayed towards zero is not wanted), so they lie with the biases behind every decayed tensor
        # and layer_grad_range and the data-parallel buckets keep their ranges
        self.layer_norm = layer_norm_config(cfg)
        if self.layer_norm:
            for i in range(self.num_layers):
                specs += [("ln%d/gamma" % i, (H,), "ln_gamma"), ("ln%d/beta" % i, (H,), "ln_beta")]
        if self.E > 0:                                                            # moe.py:33-58
            specs += [("Variable", (H, self.E), "head_w"), ("Variable_1", (self.E,), "head_b"),
                      ("Variable_2", (H, self.E * V), "head_w"), ("Variable_3", (self.E * V,), "head_b")]
        else:                                                                     # bilstm.py:238-248
            specs += [("Variable", (H, V), "head_w"), ("Variable_1", (V,), "head_b")]
        undecayed = lambda s: "bias" in s[0] or s[2] in ("ln_gamma", "ln_beta")
        decayed = [s for s in specs if not undecayed(s)]                          # graph.py:183-187
        plain = [s for s in specs if undecayed(s)]
        self.specs = decayed + plain
        self.kinds = {s[0]: s[2] for s in self.specs}
        self.shapes = {s[0]: s[1] for s in self.specs}
        self.offsets = {}
        off = 0
        for name, shape, _ in self.specs:
            if name == plain[0][0] if plain else False:
                self.n_decay = off
            self.offsets[name] = off
            off += (int(np.prod(shape)) + 3) // 4 * 4       # keep every tensor 16-byte aligned
        if not plain:
            self.n_decay = off
        self.n = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=device)
        self.grad = torch.zeros(off, dtype=torch.float32, device=device)
        self.aux = {name: torch.full(shape, float(init), dtype=torch.float32, device=device)
                    for name, shape, init in self.aux_specs}
        self._perm = gate_perm(N)
        self._inv = np.argsort(self._perm)

    def names(self):
        return [s[0] for s in self.specs]

    def _view(self, buf, name):
        shape = self.shapes[name]
        o = self.offsets[name]
        return buf[o:o + int(np.prod(shape))].view(*shape)

    def p(self, name):
        return self._view(self.flat, name)

    def g(self, name):
        return self._view(self.grad, name)

    def num_params(self):
        return sum(int(np.prod(s[1])) for s in self.specs)

    # --- TF-layout import / export (checkpoint I/O and parity tests) ---------------------------
    def _to_internal(self, name, arr):
        kind = self.kinds[name]
        if kind == "lstm_kernel":
            return arr[:, self._perm]
        if kind == "lstm_bias":
            return arr[self._perm]
        return arr

    def _to_tf(self, name, arr):
        kind = self.kinds[name]
        if kind == "lstm_kernel":
            return arr[:, self._inv]
        if kind == "lstm_bias":
            return arr[self._inv]
        return arr

    def load_tf(self, params):
        """params: dict name -> numpy array in TF layout (tf.trainable_variables shapes)."""
        missing = [n for n in self.names() if n not in params]
        if self.layer_norm and any(self.kinds[n] == "ln_gamma" for n in missing):
            raise KeyError("checkpoint has no %s: a model with layer_norm = true cannot start from a plain model's checkpoint "
                           "(no setting of ln*/gamma and ln*/beta computes what that model computed)"
                           % ", ".join(n for n in missing if self.kinds[n] == "ln_gamma"))
        if self.conv and any(self.kinds[n] == "conv_kernel" for n in missing):
            raise KeyError("checkpoint has no %s: a model with conv_layers = %d cannot start from a plain model's checkpoint "
                           "(layer 0 reads the front-end's %d columns, not the %d input columns)"
                           % (", ".join(n for n in missing if self.kinds[n] == "conv_kernel"), len(self.conv), self.D0, self.D))
        if not self.conv and "conv0/kernel" in params:
            raise KeyError("checkpoint has conv0/kernel: it was written by a model with conv_layers set, and this model (no "
                           "conv_layers key) reads the input columns directly")
        if not self.layer_norm and "ln0/gamma" in params:
            raise KeyError("checkpoint has ln0/gamma: it was written by a model with layer_norm = true, and this model (no "
                           "layer_norm key) would compute something else with its other variables")
        if missing == ["row_conv/kernel"]:
            # a plain model's checkpoint: the identity filter computes what that model computed (fine-tuning with lookahead)
            from . import tflog
            tflog.info("checkpoint has no row_conv/kernel: row convolution starts from the identity (row 0 ones, %d rows of "
                       "zeros)" % self.row_conv)
            params = dict(params)
            params["row_conv/kernel"] = row_conv_identity(self.shapes["row_conv/kernel"])
            missing = []
        if missing:
            raise KeyError("checkpoint lacks variables: %s" % missing)
        for name in self.names():
            a = np.asarray(params[name], np.float32)
            if tuple(a.shape) != tuple(self.shapes[name]):
                why = ""
                if self.time_reduce and self.kinds[name] == "lstm_kernel":
                    why = (" (time_reduce_layers = %s widens the input of those layers %d times: a plain model's checkpoint "
                           "does not fit)" % (",".join(str(l) for l in self.time_reduce), self.time_reduce_factor))
                raise ValueError("shape mismatch for %s: %s vs %s%s" % (name, a.shape, self.shapes[name], why))
            self.p(name).copy_(torch.from_numpy(np.ascontiguousarray(self._to_internal(name, a))))
        for name, shape, _ in self.aux_specs:        # moving averages: restored when the checkpoint has them
            if name in params:
                a = np.asarray(params[name], np.float32)
                if tuple(a.shape) != tuple(shape):
                    raise ValueError("shape mismatch for %s: %s vs %s" % (name, a.shape, shape))
                self.aux[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def export_tf(self, grads=False):
        out = {}
        for name in self.names():
            a = (self.g(name) if grads else self.p(name)).detach().cpu().numpy()
            out[name] = np.ascontiguousarray(self._to_tf(name, a))
        if not grads:
            for name in self.aux:
                out[name] = self.aux[name].detach().cpu().numpy().copy()
        return out

    def init_random(self, seed=None):
        """The reference's initialisers: Glorot-uniform LSTM kernels, peepholes
        and projections (TF variable-scope default), zero biases, truncated-normal heads with
        stddev 1/sqrt(num_neurons) (bilstm.py:239, sic), 1/sqrt(output_dim) (moe.py:33,48; lstm.py:333)."""
        rng = np.random.default_rng(seed)
        params = {}
        for name, shape, kind in self.specs:
            if kind in ("lstm_kernel", "proj", "peephole"):
                fan_in, fan_out = (shape[0], shape[1]) if len(shape) == 2 else (shape[0], shape[0])
                lim = math.sqrt(6.0 / (fan_in + fan_out))
                params[name] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
            elif kind == "conv_kernel":
                # Glorot-uniform over the receptive field: fan_in = 9 Cin, fan_out = 9 Cout (the biases are zeros, below)
                lim = math.sqrt(6.0 / (9 * shape[2] + 9 * shape[3]))
                params[name] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
            elif kind == "head_w":
                if self.cudnn:
                    std = 1.0 / math.sqrt(float(self.N))                           # lstm.py:105
                elif self.E > 0 or not self.blstm:
                    std = 1.0 / math.sqrt(float(self.H))
                else:
                    std = 1.0 / math.sqrt(float(self.N))
                a = rng.normal(0.0, std, size=shape)
                bad = np.abs(a) > 2 * std
                while bad.any():                                  # tf.truncated_normal: re-draw outside 2 sigma
                    a[bad] = rng.normal(0.0, std, size=int(bad.sum()))
                    bad = np.abs(a) > 2 * std
                params[name] = a.astype(np.float32)
            elif kind in ("bn_gamma", "ln_gamma"):
                params[name] = np.ones(shape, np.float32)                 # (ln: nothing drawn, like row_conv below)
            elif kind == "row_conv":
                params[name] = row_conv_identity(shape)            # nothing drawn: the other tensors are the plain model's
            else:
                params[name] = np.zeros(shape, np.float32)
        self.load_tf(params)


X3_FWD_MIN_N = int(os.environ.get("LC_X3_FWD_MIN_N", "448"))     # split-operand FORWARD recurrence above this width only


def x3_forward_recurrence(N):
    """bf16x3 mode: whether the FORWARD recurrence of an N-unit layer runs the split-operand kernel (the BPTT always does where
    one exists).  Measured, us per step at B = 32, fp32 kernel with its operands a step ahead / split-operand kernel
    (profiles/r6_x3_width_probe.txt): N = 320 1.78 / 2.12, 384 1.99 / 2.14, 448 2.64 / 2.70, 512 2.90 / 2.55 - the crossover
    lies between 448 and 512 (rounds 4-5 had measured 320 and 512 only and drawn the line at 320)."""
    return N > X3_FWD_MIN_N


_PACK_FALLBACK_LOGGED = False      # "pack_frames needs fp32" is said once per process
_PACK_REDUCE_LOGGED = False        # ... and so is "pack_frames runs padded with time_reduce_layers"

X3_FORCE = False          # tests: every eligible product on the bf16x3 kernels, whatever its size
X3_MIN_FILL = int(os.environ.get("LC_X3_MIN_FILL", "45"))     # per cent of whole 256-CU rounds (development knob)


def _x3_pays(M, N, K, split_k=False):
    """Whether an [M, K] x [K, N] product goes to the bf16x3 kernels (256 x 256 tiles, one workgroup per CU): big enough to
    amortise the operand splits, and its tiles (x K slices for the weight gradients) fill the whole rounds of 256 CUs they
    take to at least 45 %.  Round 5 measured the rule instead of inheriting the fp32 256 x 256 kernel's 90 %
    (`profiles/r5_x3_fill_sweep.txt`): a split-operand tile takes ~0.65 of an fp32 tile's time, so c2's 32000 x 1280 x 640
    products (2.44 rounds = 81 %) run 323 us against 505 us on the fp32 kernels and its 32000 x 640 x 1280 ones (1.46 rounds of
    tiles that are 5 / 6 useful) 361 against 498; in the step c2x3 goes from 26.5 to 26.0 ms and c3x3 from 64.9 to 64.0.
    Everything else stays on the fp32 kernels."""
    if X3_FORCE:
        return M >= 1 and N >= 1 and K >= 1
    if K < 64 or 2.0 * M * N * K < 2e10:
        return False
    tiles = -(-M // 256) * -(-N // 256)
    if split_k and tiles < 256:
        return K >= 4096                       # lc_gemm_bf16x3_tn slices K to whole rounds
    rounds = -(-tiles // 256)
    return tiles >= 128 and tiles * 100 >= rounds * 256 * X3_MIN_FILL


def config_keep(cfg):
    """The dropout keep probability a Model built from ``cfg`` runs with (1.0 = no dropout), without building it:
    ``dropout_rate`` while training (bilstm.py:98-101), 1.0 otherwise and for cudnnlstm (lstm.py:26-122: no DropoutWrapper)."""
    is_training = cfg.get("is_training")
    dr = cfg.get("dropout_rate")
    if dr is None or not (True if is_training is None else bool(is_training)) or cfg.get("nnet_type") == "cudnnlstm":
        return 1.0
    return float(dr)


def chunk_config(cfg):
    """(Nc, Nr) of the latency-controlled BiLSTM keys ``chunk_frames`` / ``lookahead_frames`` (extension, model frames;
    DESIGN.md 3.13), validated: (0, 0) when ``chunk_frames`` is absent or 0 - today's model -, else Nc >= 1 and Nr >= 0.
    The keys change what the model computes, so what cannot run them is refused here, never run without them."""
    def key(name):
        v = cfg.get(name)
        if v is None:
            return 0
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("%s must be a non-negative integer (model frames), got %r" % (name, v))
        return int(v)
    Nc, Nr = key("chunk_frames"), key("lookahead_frames")
    if Nc == 0:
        return 0, 0
    if cfg.get("nnet_type", "blstm") != "blstm":
        raise ValueError("chunk_frames / lookahead_frames restart the backward direction of nnet_type = blstm; nnet_type = "
                         "%s has none" % cfg.get("nnet_type"))
    cd = str(cfg.get("compute_dtype") or "fp32").lower()
    if cd not in ("fp32", "float32", "f32"):
        raise ValueError("chunk_frames / lookahead_frames are built for compute_dtype = fp32 only, got compute_dtype = %s" % cd)
    return Nc, Nr


ROW_CONV_MAX_FRAMES = 32      # the library's cap (lc_row_conv_fwd: a column group's weights live in LDS)


def row_conv_config(cfg):
    """tau of the row-convolution key ``row_conv_frames`` (extension, model frames), validated: 0 when the key
    is absent or 0 - today's model -, else an integer in 1..32 and a unidirectional nnet_type.  Like the chunk keys it changes
    what the model computes, so what cannot run it is refused here."""
    v = cfg.get("row_conv_frames")
    if v is None:
        return 0
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v > ROW_CONV_MAX_FRAMES:
        raise ValueError("row_conv_frames must be an integer in 0..%d (model frames), got %r" % (ROW_CONV_MAX_FRAMES, v))
    if v == 0:
        return 0
    if cfg.get("nnet_type", "blstm") == "blstm":
        raise ValueError("row_conv_frames gives a unidirectional model (nnet_type = lstm or cudnnlstm) lookahead; nnet_type = "
                         "blstm already reads the whole future")
    return int(v)


def layer_norm_config(cfg):
    """Whether the key ``layer_norm`` (extension) is on, validated: False when it is absent or false - today's
    model -, True for true; anything that is not a boolean is refused, and so is the key together with ``use_bn`` (two
    normalisations of the same tensor).  Like the chunk keys it changes what the model computes."""
    v = cfg.get("layer_norm")
    if v is None:
        return False
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("layer_norm must be true or false, got %r" % (v,))
    if not v:
        return False
    if cfg.get("use_bn"):
        raise ValueError("layer_norm does not combine with use_bn: both would normalise every layer's output")
    return True


def layer_norm_info_line(cfg):
    """The INFO line of nnet-init / -train / -validate / -forward / -align when the key is on, else None."""
    if not layer_norm_config(cfg):
        return None
    L = int(cfg["num_layers"])
    return ("layer normalisation: layer_norm = true: the outputs of layers 0..%d are normalised over their columns (both "
            "directions of a blstm layer together), dropout behind it; eps = %g" % (L - 1, ops.LN_EPS))


CONV_MAX_LAYERS = 3


def conv_config(cfg):
    """The layers of the convolutional front-end (extension keys ``conv_layers`` / ``conv_channels`` / ``conv_bins``; DESIGN.md
    3.20), validated: () when ``conv_layers`` is absent or 0 - today's model, and the other two keys are then not read -, else
    one (Cin, Cout, F, Fo) per layer: layer k maps F_k bins to ceil(F_k / 2) bins and to ``conv_channels`` channels, the first
    one reading ``input_dim / conv_bins`` channels of ``conv_bins`` bins.  Like the chunk keys it changes what the model
    computes, so what cannot run it is refused here, by name."""
    def integer(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
        return int(v)
    v = cfg.get("conv_layers")
    if v is None:
        return ()
    n = integer("conv_layers", v)
    if n < 0 or n > CONV_MAX_LAYERS:
        raise ValueError("conv_layers must be in 0..%d (0: off), got %r" % (CONV_MAX_LAYERS, v))
    if n == 0:
        return ()
    Cc = cfg.get("conv_channels")
    Cc = 32 if Cc is None else integer("conv_channels", Cc)
    if Cc < 8 or Cc > ops.CONV_MAX_CHANNELS or Cc % 8:
        raise ValueError("conv_channels must be a multiple of 8 in 8..%d, got %r" % (ops.CONV_MAX_CHANNELS, Cc))
    D = integer("input_dim", cfg.get("input_dim"))
    F = cfg.get("conv_bins")
    F = D if F is None else integer("conv_bins", F)
    if F < 1 or F > ops.CONV_MAX_BINS or D % F:
        raise ValueError("conv_bins must be in 1..%d and divide input_dim = %d, got %r" % (ops.CONV_MAX_BINS, D, F))
    if D // F > ops.CONV_MAX_CHANNELS:
        raise ValueError("conv_bins = %d leaves input_dim / conv_bins = %d input channels, more than %d"
                         % (F, D // F, ops.CONV_MAX_CHANNELS))
    if (cfg.get("left_context") or 0) or (cfg.get("right_context") or 0):
        raise ValueError("conv_layers does not combine with left_context / right_context (%r, %r): the convolution supplies the "
                         "context, and a spliced input has no frequency axis to convolve"
                         % (cfg.get("left_context"), cfg.get("right_context")))
    if cfg.get("use_bn"):
        raise ValueError("conv_layers does not combine with use_bn: the batch normalisation of the input is not built in front "
                         "of the convolution")
    if cfg.get("pack_frames"):
        raise ValueError("conv_layers does not combine with pack_frames = true: the convolution reads neighbouring frames of "
                         "the padded layout")
    cd = str(cfg.get("compute_dtype") or "fp32").lower()
    if cd not in ("fp32", "float32", "f32"):
        raise ValueError("conv_layers is built for compute_dtype = fp32 only, got compute_dtype = %s (the conv passes and the "
                         "layer-0 dX they need are fp32)" % cd)
    layers, Cin = [], D // F
    for _ in range(n):
        Fo = ops.conv_out_bins(F)
        layers.append((Cin, Cc, F, Fo))
        Cin, F = Cc, Fo
    return tuple(layers)


def conv_info_line(cfg):
    """The INFO line of nnet-init / -train / -validate / -forward / -align when the key is on, else None."""
    layers = conv_config(cfg)
    if not layers:
        return None
    params = sum(9 * Cin * Cc + Cc for Cin, Cc, _, _ in layers)
    return ("convolutional front-end: conv_layers = %d, conv_channels = %d, conv_bins = %d: %d input channels, bins %s, layer 0 "
            "reads %d columns; %d parameters added; every logit reads %d more frames on each side"
            % (len(layers), layers[0][1], layers[0][2], layers[0][0],
               " -> ".join(str(f) for f in [layers[0][2]] + [l[3] for l in layers]), layers[-1][3] * layers[-1][1], params,
               len(layers)))


TIME_REDUCE_FACTORS = (2, 4)      # the library's range of r (lc_time_reduce_fwd)


def time_reduce_config(cfg):
    """(layers, r) of the pyramidal-BiLSTM keys ``time_reduce_layers`` / ``time_reduce_factor`` (extension),
    validated: ``layers`` the ascending tuple of 0-based indices of the layers whose INPUT joins r consecutive frames of the
    layer below into one frame r times as wide, each in 1 .. num_layers - 1; ((), 2) when the first key is absent or 0 -
    today's model, and the factor is then not read.  The key comes from ``parse_config`` as an int (one index) or a string (a
    comma list).  Like the chunk keys it changes what the model computes, so what cannot run it is refused here."""
    v = cfg.get("time_reduce_layers")
    if v is None or (isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v == 0):
        return (), 2
    bad = ValueError("time_reduce_layers must be 0 (off) or strictly ascending layer indices in 1 .. num_layers - 1 (one "
                     "integer or a comma list), got %r" % (v,))
    if isinstance(v, bool):
        raise bad
    if isinstance(v, (int, np.integer)):
        layers = [int(v)]
    elif isinstance(v, str):
        try:
            layers = [int(tok) for tok in v.split(",")]
        except ValueError:
            raise bad from None
    elif isinstance(v, (list, tuple)) and all(isinstance(e, (int, np.integer)) and not isinstance(e, bool) for e in v):
        layers = [int(e) for e in v]
    else:
        raise bad
    L = int(cfg["num_layers"])
    if not layers or any(l < 1 or l > L - 1 for l in layers) or any(a >= b for a, b in zip(layers, layers[1:])):
        raise ValueError("time_reduce_layers must be strictly ascending layer indices in 1 .. num_layers - 1 = %d, got %r"
                         % (L - 1, v))
    r = cfg.get("time_reduce_factor")
    r = 2 if r is None else r
    lo, hi = TIME_REDUCE_FACTORS
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r < lo or r > hi:
        raise ValueError("time_reduce_factor (read with time_reduce_layers) must be an integer in %d..%d, got %r" % (lo, hi, r))
    if cfg.get("nnet_type", "blstm") != "blstm":
        raise ValueError("time_reduce_layers widens a layer's input, which nnet_type = blstm alone allows; the residual and "
                         "batch-norm rules of nnet_type = %s tie input width to output width" % cfg.get("nnet_type"))
    cd = str(cfg.get("compute_dtype") or "fp32").lower()
    if cd not in ("fp32", "float32", "f32"):
        raise ValueError("time_reduce_layers is built for compute_dtype = fp32 only, got compute_dtype = %s (its shadow-only "
                         "activations have no fp32 layer output to re-lay)" % cd)
    if chunk_config(cfg)[0] > 0:
        raise ValueError("time_reduce_layers does not combine with chunk_frames / lookahead_frames (the chunk layout is built "
                         "at one frame rate)")
    return tuple(layers), int(r)


def time_reduce_info_line(cfg):
    """The INFO line of nnet-init / -train / -validate / -forward when the key is on, else None."""
    layers, r = time_reduce_config(cfg)
    if not layers:
        return None
    R = r ** len(layers)
    return ("pyramidal BiLSTM: time_reduce_layers = %s, time_reduce_factor = %d: R = %d, the logits come once per %d model "
            "frames (%d raw frames)" % (",".join(str(l) for l in layers), r, R, R, R * max(int(cfg.get("subsample") or 0), 1)))


def row_conv_identity(shape):
    """The filter that leaves the model as it was: row 0 ones, the lookahead rows zeros."""
    w = np.zeros(shape, np.float32)
    w[0] = 1.0
    return w


def row_conv_horizon_raw(cfg):
    """(model frames, raw frames) the logits of a row-convolution model read past their own frame: tau, and that times the
    subsampling factor plus the splice's right context."""
    tau = row_conv_config(cfg) + len(conv_config(cfg))         # (the front-end reads one more model frame per layer)
    return tau, tau * max(int(cfg.get("subsample") or 0), 1) + int(cfg.get("right_context") or 0)


def row_conv_info_line(cfg):
    """The INFO line of nnet-train / -validate / -forward / -align when the key is on, else None."""
    tau = row_conv_config(cfg)
    if not tau:
        return None
    ahead, raw = row_conv_horizon_raw(cfg)
    return ("row convolution: row_conv_frames = %d: logits read %d model frames (%d raw frames) past their own"
            % (tau, ahead, raw))


def chunk_horizon(num_layers, Nc, Nr, c=0, T=None):
    """H_L(c): the logits of chunk c of an L-layer latency-controlled BiLSTM (no splicing) read no input frame at or beyond
    it.  H_1 = (c + 1) Nc + Nr; a layer above reads its input up to H_l - 1, whose backward outputs come from the chunk that
    frame lies in: H_{l+1} = ((H_l - 1) // Nc + 1) Nc + Nr.  Clipped to T when given."""
    clip = (lambda h: h) if T is None else (lambda h: min(h, T))
    H = clip((c + 1) * Nc + Nr)
    for _ in range(num_layers - 1):
        H = clip(((H - 1) // Nc + 1) * Nc + Nr)
    return H


def chunk_horizon_raw(cfg):
    """(model frames, raw frames) a chunk's logits look past its end at worst, for the INFO line of the command-line tools:
    H_L(0) - Nc, and that times the subsampling factor plus the splice's right context."""
    Nc, Nr = chunk_config(cfg)
    h = chunk_horizon(cfg["num_layers"], Nc, Nr) - Nc + len(conv_config(cfg))    # (+ one model frame per front-end layer)
    return h, h * max(int(cfg.get("subsample") or 0), 1) + int(cfg.get("right_context") or 0)


def chunk_info_line(cfg):
    """The INFO line of nnet-train / -validate / -forward / -align when the mode is on, else None."""
    Nc, Nr = chunk_config(cfg)
    if not Nc:
        return None
    h, raw = chunk_horizon_raw(cfg)
    return ("latency-controlled BiLSTM: chunk_frames = %d, lookahead_frames = %d, %d layers: a chunk's logits read %d model "
            "frames (%d raw frames) past its end" % (Nc, Nr, cfg["num_layers"], h, raw))


class Model:
    """Forward / backward of the stack on one batch.  ``x`` is time-major ``[T,B,D]`` on the GPU,
    zero beyond each utterance's length (the pipeline's padding value, nnet/pipeline.py:44)."""

    def __init__(self, cfg, device="cuda", seed=None):
        self.cfg = dict(cfg)
        # Extension keys chunk_frames = Nc, lookahead_frames = Nr (model frames; absent or Nc = 0: off): the latency-controlled
        # BiLSTM - every layer's backward direction restarts from a zero state in each chunk of Nc frames after Nr lookahead
        # frames, as the same reverse recurrence on a re-laid-out batch of ceil(T / Nc) * B rows (lc_chunk_gather /
        # lc_chunk_fold).  Parameters and checkpoints are the plain model's.  fp32 only; refused otherwise.
        self.chunk, self.lookahead = chunk_config(self.cfg)
        # Extension key row_conv_frames = tau (model frames; absent or 0: off, the plain model to the bit): the uni-LSTM's
        # lookahead - one depthwise filter over the next tau frames of the top layer's output (after its batch norm), in front
        # of the head (lc_row_conv_fwd / lc_row_conv_bwd).  Always fp32; one more parameter, row_conv/kernel.
        self.row_conv = row_conv_config(self.cfg)
        # Extension keys time_reduce_layers = l[,m,...], time_reduce_factor = r (absent or 0: off, the plain model to the bit):
        # the pyramidal BiLSTM - the input of each listed layer is r consecutive frames of the layer below side by side
        # (lc_time_reduce_fwd / lc_time_reduce_bwd), and everything from that layer up runs on ceil(T / r)
        # frames with lengths ceil(len / r).  The listed layers' kernels are wider: a plain checkpoint does not fit.
        self.time_reduce, self.time_reduce_factor = time_reduce_config(self.cfg)
        self.time_factor = self.time_reduce_factor ** len(self.time_reduce)      # R: input frames per logit frame, 1 when off
        # Extension key layer_norm = true (absent or false: off, the plain model to the bit): every layer's output is normalised
        # over its columns, with a gain and an offset ln{i}/gamma, ln{i}/beta, and the DropoutWrapper mask moves behind the
        # normalisation (lc_layer_norm_fwd / lc_layer_norm_bwd).  A plain checkpoint is refused by name.
        self.layer_norm = layer_norm_config(self.cfg)
        # Extension keys conv_layers = n, conv_channels = Cc, conv_bins = F (absent or 0: off, the plain model to the bit): the
        # convolutional front-end - n layers of 3 x 3 convolution over (time, frequency) with bias and ReLU, frequency stride 2,
        # between x and layer 0, which reads the last one's [F_n * Cc] columns (lc_conv_fwd / lc_conv_bwd).
        # Frame counts and lengths do not change.  fp32, no splice, no use_bn, no pack_frames: refused by name otherwise.
        self.conv = conv_config(self.cfg)
        self.device = torch.device(device)
        self.ps = ParamStore(self.cfg, self.device)
        self.ps.init_random(seed)
        is_training = self.cfg.get("is_training")
        self.is_training = True if is_training is None else bool(is_training)
        self.keep = config_keep(self.cfg)
        mt = self.cfg.get("moe_temp")
        self.tau = 10.0 if mt is None else float(mt)                                 # bilstm.py:74-76
        self.forget_bias = 5.0 if self.ps.blstm else 1.0                             # bilstm.py:133 / TF default
        if self.ps.cudnn:
            self.forget_bias = 0.0                       # CudnnCompatibleLSTMCell: LSTMBlockCell(forget_bias=0)
        # Extension key (not in the reference): compute_dtype = bf16 selects BASELINE config c5 - every product
        # with an activation operand (gate/projection/head GEMMs, their gradients, the recurrent step) rounds
        # its operands to bf16 and accumulates in fp32; weights, state, CTC and the optimizer stay fp32.
        cd = str(self.cfg.get("compute_dtype") or "fp32").lower()
        if cd not in ("fp32", "float32", "f32", "bf16", "bfloat16", "bf16x3"):
            raise ValueError("compute_dtype must be fp32, bf16x3 or bf16, got %r" % cd)
        self.bf16 = cd in ("bf16", "bfloat16")
        # compute_dtype = bf16x3 (extension): fp32 semantics on the bf16 matrix cores - the products with an activation
        # operand split both fp32 operands exactly into three bf16 terms and accumulate the six significant term products
        # in fp32 (lc_split_bf16x3 + lc_gemm_bf16x3_nt; error against float64 no larger than the fp32 MFMA kernels').
        # The recurrence, CTC, weight-only products and the optimizer are the fp32 mode's.
        self.x3 = cd == "bf16x3"
        # bf16 mode, second stage: operands go through bf16 shadow copies (faster loader); off -> converting loader only
        sh = self.cfg.get("bf16_shadows")
        self.use_shadows = self.bf16 and (True if sh is None else bool(sh))
        self._shadows = {}
        self.saved = None
        # Small fp32 models run each layer's BPTT as one persistent launch that is bound by its exchange latency, not by
        # the matrix pipe: the weight-gradient GEMMs of layer i then run on a second (low-priority)
        # stream under the BPTT of layer i-1.  (For the big model the same overlap was measured twice and lost: its
        # step kernels are MFMA-bound.)  LC_OVERLAP_WGRAD=0 switches it off.
        import os
        self.overlap_wgrad = (not self.bf16 and self.ps.N <= 512 and self.ps.N % 16 == 0
                              and os.environ.get("LC_OVERLAP_WGRAD", "1") != "0")
        # (Wide layers - XCD-pair BPTT, nothing runs beside it -: a layer's weight-gradient GEMMs on the second stream BESIDE
        # its dX GEMMs, joined in front of the next BPTT, so that one product's last partial round of tiles fills with the
        # other's first, was measured at c4 in round 4: 187.7 / 187.9 k frames/s against 188.6 / 188.9 k - dropped.)
        self._side = None
        # (bf16x3 mode: a split-operand GEMM workgroup - 128 KB of LDS, two 200-register waves per SIMD - cannot share a CU
        # with a workgroup of the persistent BPTT the way an fp32 one can, and takes 642 instead of 373 us per product beside
        # it; the step is nevertheless shorter with them: c2x3 25.2 vs 25.7 ms, c3x3 65.0 vs 68.8 on one box.
        # LC_X3_SIDE_WGRAD=f32 keeps the side-stream products on the fp32 kernels.)
        self.x3_side_f32 = os.environ.get("LC_X3_SIDE_WGRAD", "x3") == "f32"
        self.fuse_dx = os.environ.get("LC_FUSE_DX", "1") != "0"       # one dX product per bidirectional layer (backward; f32 and bf16)
        # bf16: the recurrences store hs / dz ONLY as the bf16 shadows every product of the step reads (no fp32 copy), where
        # every consumer is known to take the natural shadow (`_shadow_only`); LC_C5_SHADOW_ONLY=0 writes both
        self.shadow_only = os.environ.get("LC_C5_SHADOW_ONLY", "1") != "0"
        # development / bisection knob (tools/x3_truth.py): which recurrences of the bf16x3 mode run the split-operand kernels -
        # "both" (default), "fwd", "bwd" or "none" (round 3's mode: split-operand products around fp32 recurrences)
        rec = os.environ.get("LC_X3_REC", "both")
        self.x3_rec_fwd = self.x3 and rec in ("both", "fwd")
        self.x3_rec_bwd = self.x3 and rec in ("both", "bwd")
        # DropoutWrapper masks (and the bf16 shadows of what they produce) ride in the epilogue of the product that
        # writes the masked matrix (lc_gemm_next_epilogue); LC_FUSE_DROPOUT=0 -> separate lc_dropout_scale passes
        self.fuse_dropout = os.environ.get("LC_FUSE_DROPOUT", "1") != "0"
        # Extension key pack_frames (default off; LC_PACK_FRAMES=1|0 overrides the config): on a ragged batch the products that
        # read a layer's input - zx, dKx, dX - run on a packed copy of the live frames (lc_pack_rows / lc_unpack_rows, DESIGN.md
        # section 2); recurrences, projection, head, CTC stay on the padded rows.  fp32 only: the bf16 modes read their operands
        # through shadows (bf16: shadow-ONLY activations) that have no packed form yet - they log one line and run padded.
        pf = os.environ.get("LC_PACK_FRAMES")
        self.pack_frames = bool(self.cfg.get("pack_frames") or False) if pf is None else pf != "0"
        if self.pack_frames and (self.bf16 or self.x3):
            global _PACK_FALLBACK_LOGGED
            if not _PACK_FALLBACK_LOGGED:
                _PACK_FALLBACK_LOGGED = True
                from . import tflog
                tflog.info("pack_frames is built for compute_dtype = fp32 only; compute_dtype = %s runs on the padded rows" % cd)
            self.pack_frames = False
        if self.pack_frames and self.conv:
            # (LC_PACK_FRAMES=1 over a config without the key; the key itself is refused by conv_config)
            from . import tflog
            tflog.info("pack_frames does not combine with conv_layers; the model runs on the padded rows")
            self.pack_frames = False
        if self.pack_frames and self.time_reduce:
            # (the frame map is built at one frame rate)
            global _PACK_REDUCE_LOGGED
            if not _PACK_REDUCE_LOGGED:
                _PACK_REDUCE_LOGGED = True
                from . import tflog
                tflog.info("pack_frames is built for one frame rate; with time_reduce_layers the model runs on the padded rows")
            self.pack_frames = False
        self.packed = False         # what the last forward() did: True = the input products ran on packed frames
        self._frame_map = None       # (key, the lengths the key was made from, FrameMap) of the last ragged batch

    def lookahead_horizon(self):
        """Latency-controlled mode: the worst-case number of model frames past a chunk's end that its logits read,
        H_L(0) - Nc (``chunk_horizon``); None when the mode is off (the whole utterance).  A row-convolution model
        (unidirectional): tau, the model frames its logits read past their own.  Each layer of the convolutional front-end
        adds one model frame to either."""
        if self.row_conv:
            return self.row_conv + len(self.conv)
        if not self.chunk:
            return None
        return chunk_horizon(self.ps.num_layers, self.chunk, self.lookahead) - self.chunk + len(self.conv)

    def output_frames(self, T):
        """Frames of the logits for T input frames: T with ceil(. / r) applied once per reduced layer (= ceil(T / R))."""
        T = int(T)
        for _ in self.time_reduce:
            T = ops.time_reduce_frames(T, self.time_reduce_factor)
        return T

    def output_lengths(self, seq_len):
        """The lengths the logits have for input lengths ``seq_len``: ceil(len / R).  A device tensor is answered on its
        device with integer ops (no synchronisation), anything else as a numpy int32 array.  ``seq_len`` itself when the
        model has no reduction."""
        for _ in self.time_reduce:
            seq_len = ops.time_reduce_lengths(seq_len, self.time_reduce_factor)
        return seq_len

    def frame_map(self, seq_len, T, B, seq_len_host=None):
        """The FrameMap of this batch, built once per distinct batch.  With ``seq_len_host`` (the lengths as a host array: a
        caller that has them, CTCGraph.step, passes them and no synchronisation happens) the last map is re-used while the
        array compares equal.  Without it the key is the device tensor's identity and state, (data_ptr, _version, T, B): a loop
        that re-uses one tensor (step_device, bench.py) pays the device-to-host copy once, an in-place change of the lengths
        bumps _version, and the entry keeps the tensor alive so that its address cannot be handed to another one."""
        from .frames import FrameMap
        hit = self._frame_map
        if seq_len_host is not None:
            host = np.ascontiguousarray(seq_len_host, dtype=np.int32)
            if hit is not None and hit[0] == ("host", T, B) and np.array_equal(hit[1], host):
                return hit[2]
            self._frame_map = (("host", T, B), host.copy(), FrameMap(host, T, B))
        else:
            key = (seq_len.data_ptr(), seq_len._version, T, B)
            if hit is not None and hit[0] == key:
                return hit[2]
            self._frame_map = (key, seq_len, FrameMap(seq_len.cpu().numpy(), T, B))
        return self._frame_map[2]

    # ---- products with an activation operand: follow compute_dtype (weight-only products stay ops.gemm / fp32)
    def _shadow(self, t, tr):
        """bf16 shadow of the fp32 matrix / view ``t`` (transposed copy if ``tr``), made once per step.  The cache
        entry keeps ``t`` alive, so its address cannot be handed to another tensor while the shadow is valid; every
        operand is cast only after its last in-place modification of the step."""
        key = (t.data_ptr(), tuple(t.shape), t.stride(0), bool(tr))
        hit = self._shadows.get(key)
        if hit is None:
            nat, trn = ops.cast_bf16(t, nat=not tr, tr=tr)
            hit = (t, trn if tr else nat)
            self._shadows[key] = hit
        return hit[1]

    def _shadow3(self, t, tr=False):
        """x3 shadow (hi | mid | lo bf16 terms, lc_split_bf16x3) of the fp32 matrix / view ``t`` - of its transpose if ``tr``
        (weights only) -, made once per step under the same rules as ``_shadow``."""
        key = (t.data_ptr(), tuple(t.shape), t.stride(0), bool(tr), "x3")
        hit = self._shadows.get(key)
        if hit is None:
            hit = (t, ops.split_bf16x3(ops.transpose(t) if tr else t))
            self._shadows[key] = hit
        return hit[1]

    def _shadow_pad256(self, t):
        """Natural bf16 shadow of the NARROW fp32 matrix ``t`` [rows, C < 256] in a zero-padded [rows, 256] buffer: a K-major
        operand of the 256 x 256 TN kernel (the 40-wide input's and the 44-wide head's weight gradients), once per step."""
        key = (t.data_ptr(), tuple(t.shape), t.stride(0), False, "pad256")
        hit = self._shadows.get(key)
        if hit is None:
            buf = torch.zeros((t.shape[0], 256), dtype=torch.bfloat16, device=t.device)
            ops.cast_bf16(t, out_nat=buf)
            hit = (t, buf)
            self._shadows[key] = hit
        return hit[1]

    def _shadow_only(self, rows, I):
        """Whether the fp32 hs / dz of a layer with input width I may stay unwritten: bf16 mode with shadows, a plain BiLSTM
        layer, and shapes for which EVERY product that reads hs or dz takes its natural bf16 shadow (projection, dproj, dR, dKx,
        dX - see _mm and backward): layer widths in whole 256-tiles, and for a narrow input (layer 0) the padded K-major route,
        which needs rows >= 4096.  The library honours the request in its full-width kernel (N = 1024) and ignores it elsewhere."""
        ps = self.ps
        return bool(self.shadow_only and self.bf16 and self.use_shadows and ps.blstm and not ps.use_bn and not ps.layer_norm and ps.P
                    and ps.N % 256 == 0 and ps.Pout % 256 == 0 and rows % 256 == 0 and rows >= 4096
                    and (I % 256 == 0 or I < 256))

    def _adopt_shadow(self, t, shadow):
        """Registers ``shadow`` (bf16, same orientation, written by the kernel that produced ``t``) as the step's
        shadow of the fp32 matrix ``t``: the next ``_shadow(t, tr=False)`` takes it instead of casting."""
        self._shadows[(t.data_ptr(), tuple(t.shape), t.stride(0), False)] = (t, shadow)

    def _mm(self, A, B, ta=False, tb=False, out=None, alpha=1.0, beta=0.0, bias=None, epilogue=None, x3_ok=True):
        """op(A) @ op(B) (+bias), fp32 or - compute_dtype = bf16 - with bf16 operands: through bf16 shadow copies
        in NT form (lc_cast_bf16 + lc_gemm_bf16_nt) when K allows 16-byte operand rows, else with the converting
        loader (lc_gemm_bf16); both round the same operands the same way."""
        if self.x3 and not ta and A.dim() == 2 and B.dim() == 2 and _x3_pays(A.shape[0], B.shape[0] if tb else B.shape[1], A.shape[1]):
            # activation rows x weight: A's x3 shadow as it lies, the weight's with k contiguous (B itself for op(B) = B^T)
            return ops.gemm_bf16x3_nt(self._shadow3(A), self._shadow3(B, tr=not tb), A.shape[1], out=out, alpha=alpha,
                                      beta=beta, bias=bias, epilogue=epilogue)
        if (self.x3 and x3_ok and ta and not tb and A.dim() == 2 and B.dim() == 2 and epilogue is None
                and _x3_pays(A.shape[1], B.shape[1], A.shape[0], split_k=True)):
            # X^T dZ: both activations K-major - the shadows the forward / dX products already made
            return ops.gemm_bf16x3_tn(self._shadow3(A), self._shadow3(B), A.shape[1], B.shape[1], out=out, alpha=alpha,
                                      beta=beta, bias=bias)
        if not self.bf16:
            return ops.gemm(A, B, ta=ta, tb=tb, out=out, alpha=alpha, beta=beta, bias=bias, epilogue=epilogue)
        K = A.shape[0] if ta else A.shape[1]
        if (self.use_shadows and ta and not tb and A.dim() == 2 and B.dim() == 2 and A.shape[1] % 256 == 0
                and B.shape[1] % 256 == 0 and A.stride(0) % 8 == 0 and B.stride(0) % 8 == 0):
            # X^T dZ with both layer widths in whole 256-tiles: the K-major kernel on the NATURAL shadows (transposing
            # LDS reads) - no transposed copy of either activation is ever made
            return ops.gemm_bf16_tn(self._shadow(A, tr=False), self._shadow(B, tr=False), out=out, alpha=alpha,
                                    beta=beta, bias=bias, epilogue=epilogue)
        if (self.use_shadows and ta and not tb and A.dim() == 2 and B.dim() == 2 and beta == 0.0 and bias is None
                and epilogue is None and K >= 4096
                and ((A.shape[1] % 256 == 0 and B.shape[1] < 256) or (B.shape[1] % 256 == 0 and A.shape[1] < 256))):
            # X^T dZ with ONE narrow side (the 40-wide input layer, the 44-wide head): the K-major kernel on the wide
            # operand's natural shadow and a zero-padded 256-column shadow of the narrow one, the valid block copied out -
            # instead of a TRANSPOSED bf16 copy of the wide activation (0.26 - 0.5 ms each at c5's sizes) for the NT form.
            # Same operand roundings, another summation order.
            if A.shape[1] < 256:
                full = ops.gemm_bf16_tn(self._shadow_pad256(A), self._shadow(B, tr=False), alpha=alpha)
                res = full[:A.shape[1]]
            else:
                full = ops.gemm_bf16_tn(self._shadow(A, tr=False), self._shadow_pad256(B), alpha=alpha)
                res = full[:, :B.shape[1]]
            if out is None:
                return res.contiguous()
            out.copy_(res)
            return out
        if (self.use_shadows and not ta and not tb and A.dim() == 2 and B.dim() == 2 and A.shape[0] % 256 == 0
                and B.shape[1] % 256 == 0 and K % 64 == 0 and A.stride(0) % 8 == 0 and B.stride(0) % 8 == 0):
            # X . W with whole 256-tiles: activation AND weight in their natural layouts (no transposed weight copy)
            return ops.gemm_bf16_nn(self._shadow(A, tr=False), self._shadow(B, tr=False), out=out, alpha=alpha,
                                    beta=beta, bias=bias, epilogue=epilogue)
        if self.use_shadows and K % 8 == 0 and A.dim() == 2 and B.dim() == 2:
            return ops.gemm_bf16_nt(self._shadow(A, tr=ta), self._shadow(B, tr=not tb), out=out, alpha=alpha,
                                    beta=beta, bias=bias, K=K, epilogue=epilogue)
        return ops.gemm(A, B, ta=ta, tb=tb, out=out, alpha=alpha, beta=beta, bias=bias, bf16=True, epilogue=epilogue)

    # ------------------------------------------------------------------------------------ helpers
    def _cell(self, prefix):
        ps = self.ps
        k = ps.p(prefix + "/kernel")
        I = k.shape[0] - ps.Pout
        return dict(Kx=k[:I], Kh=k[I:], bias=ps.p(prefix + "/bias"),
                    w_f=ps.p(prefix + "/w_f_diag") if ps.peep else None,
                    w_i=ps.p(prefix + "/w_i_diag") if ps.peep else None,
                    w_o=ps.p(prefix + "/w_o_diag") if ps.peep else None,
                    proj=ps.p(prefix + "/projection/kernel") if ps.P else None, I=I, prefix=prefix)

    def _prefixes(self, i):
        if self.ps.blstm:
            return ["fd%d/frnn%d" % (i, i), "bd%d/brnn%d" % (i, i)]
        if self.ps.cudnn:
            return [CUDNN_CELL % i]
        return ["drnn%d/lstm_cell" % i]

    # ------------------------------------------------------------------------------------ forward
    def forward(self, x, seq_len, drop_seed=0, seq_len_host=None):
        """x [T,B,D] f32 cuda, seq_len [B] int32 cuda -> logits [T,B,V] (time-major; with time_reduce_layers
        [output_frames(T),B,V], whose lengths are output_lengths(seq_len)).  seq_len_host: the same lengths as a
        host array, if the caller has them (pack_frames then needs no device-to-host copy for a new batch)."""
        ps = self.ps
        self._shadows.clear()                       # parameters moved since the last step; activations are new
        T, B, D = x.shape
        assert D == ps.D, (D, ps.D)
        rows, N, P = T * B, ps.N, ps.Pout
        dev = x.device
        # pack_frames: a batch with dead frames runs its input products on the M live rows (rounded up to Mp); one without
        # (M == T * B; or with no live frame at all) takes the padded path untouched.  The test is M, not Mp: at a few frames
        # Mp, a multiple of 256, can exceed T * B and the packed path is still the one asked for.
        fm = self.frame_map(seq_len, T, B, seq_len_host) if self.pack_frames else None
        self.packed = fm is not None and 0 < fm.M < rows
        pk_rows, pk_inverse = fm.device(dev) if self.packed else (None, None)
        inp = x.reshape(rows, D)
        # the convolutional front-end: each layer's input and output are kept for its backward pass; the first layer reads the
        # loader's layout (channels as blocks of F bins), the others what the layer below wrote.  D0: what layer 0 reads
        conv_saved = []
        for k, (_, _, F, _) in enumerate(self.conv):
            y = ops.conv_fwd(inp, ps.p("conv%d/kernel" % k), ps.p("conv%d/bias" % k), seq_len, T, B, F, group_major=k == 0)
            conv_saved.append(dict(x=inp, y=y, F=F, group_major=k == 0))
            inp = y
        D0 = ps.D0
        bn_saved = {}
        chunked = self.chunk > 0
        if chunked:
            _, Tc, Bc = ops.chunk_shape(T, B, self.chunk, self.lookahead)
            len_c = ops.chunk_lengths(seq_len, T, self.chunk, self.lookahead)

        def batch_norm(name, t):
            y, mean, var = ops.bn_forward(t, ps.p(name + "/gamma"), ps.p(name + "/beta"), self.is_training,
                                          ps.aux[name + "/moving_mean"], ps.aux[name + "/moving_variance"])
            bn_saved[name] = dict(x=t, mean=mean, var=var)
            return y

        if ps.use_bn:
            inp = batch_norm("drnn_bn_0_0", inp)                                      # lstm.py:271-277
        layers = []
        # from here on T, rows and seq_len are the CURRENT layer's: a reduced layer changes all three
        for i in range(ps.num_layers):
            reduced = i in self.time_reduce
            if reduced:
                # r frames of the layer below side by side (a fresh fp32 tensor; dead frames and the cut-short last group +0),
                # and this layer and everything above it on ceil(T / r) frames; the lengths stay on the device
                r = self.time_reduce_factor
                inp = ops.time_reduce_fwd(inp, seq_len, T, B, r)
                seq_len = ops.time_reduce_lengths(seq_len.clamp(0, T), r)
                T = ops.time_reduce_frames(T, r)
                rows = T * B
            cells = [self._cell(p) for p in self._prefixes(i)]
            ndir = len(cells)
            Y = torch.empty((rows, ndir * P), dtype=torch.float32, device=dev)
            dirs = []
            # (the two directions' zx products on two streams - so that one's first round of tiles fills the other's partial
            # last one - measured in round 6 at c4: 338.7 / 338.7 against 340.9 / 338.7 ms; not taken, like round 4's attempt
            # with the weight gradients)
            inp_packed = ops.pack_rows(inp, pk_rows) if self.packed else None       # [Mp, I]: live frames, zero tail rows
            for d, c in enumerate(cells):
                if self.packed:
                    # live rows only; the dead rows of zx are zero instead of the bias: the recurrences select them away
                    zx = ops.unpack_rows(self._mm(inp_packed, c["Kx"], bias=c["bias"]), pk_inverse)
                else:
                    zx = self._mm(inp, c["Kx"], bias=c["bias"])                      # hoisted x_t.Kx + b
                R = ops.gemm(c["proj"], c["Kh"]) if c["proj"] is not None else c["Kh"]
                # (chunked backward direction: its cell state exists in the chunk layout only)
                cs = None if chunked and d == 1 else torch.empty((rows, N), dtype=torch.float32, device=dev)
                hs = torch.empty((rows, N), dtype=torch.float32, device=dev)
                dirs.append(dict(zx=zx, R=R, w_f=c["w_f"], w_i=c["w_i"], w_o=c["w_o"], cs=cs, hs=hs,
                                 reverse=(d == 1)))
                if self.bf16 and self.use_shadows and c["proj"] is not None and N % 8 == 0:
                    # the projection reads hs as a bf16 shadow: let the recurrence write it in the same pass
                    dirs[-1]["hs_bf16"] = torch.empty((rows, N), dtype=torch.bfloat16, device=dev)
                    dirs[-1]["shadow_only"] = self._shadow_only(rows, c["I"])
            # (split-operand mode, widths up to 320: the fp32 forward recurrence is the faster one since its operands are
            # requested a step ahead - 1.77 against 2.11 us per step at N = 320, 1.44 / 1.72 at 256; from 512 up the
            # split-operand kernel leads, 2.56 against 2.86: profiles/r5_persist_probe_ahead.txt)
            if chunked:
                # latency-controlled: the forward direction as it is; the backward direction on the chunked batch - Bc rows
                # of Tc frames, each with its own length, from a zero state - and its kept frames folded back
                fd, bd = dirs
                ops.lstm_fwd([fd], seq_len, T, B, N, self.forget_bias)
                ck = dict(zx=ops.chunk_gather(bd["zx"], T, B, self.chunk, self.lookahead), R=bd["R"], w_f=bd["w_f"],
                          w_i=bd["w_i"], w_o=bd["w_o"], cs=torch.empty((Tc * Bc, N), dtype=torch.float32, device=dev),
                          hs=torch.empty((Tc * Bc, N), dtype=torch.float32, device=dev), reverse=True)
                ops.lstm_fwd([ck], len_c, Tc, Bc, N, self.forget_bias)
                ops.chunk_fold(ck["hs"], T, B, self.chunk, self.lookahead, out=bd["hs"])
                bd["chunked"], bd["zx"] = ck, None          # the padded zx is spent: the gates live in the chunk layout
            else:
                ops.lstm_fwd(dirs, seq_len, T, B, N, self.forget_bias, bf16=self.bf16,
                             x3=self.x3_rec_fwd and x3_forward_recurrence(N))
            for dd in dirs:
                if dd.get("hs_bf16") is not None:
                    self._adopt_shadow(dd["hs"], dd["hs_bf16"])
            residual = (i == 0 and D0 == 2 * P) if ps.blstm else False              # bilstm.py:199
            # DropoutWrapper on each direction (layer_norm: Y stays unmasked, the mask goes on the normalised output below)
            drop = ps.blstm and self.keep < 1.0 and not ps.layer_norm
            # bf16 path: the pass that applies the mask also writes the bf16 shadow the next product reads
            # (round 6: without dropout too - inference, parity runs - when every direction has a projection product to carry it)
            Y16 = (torch.empty((rows, ndir * P), dtype=torch.bfloat16, device=dev)
                   if (drop or (ps.blstm and all(c_["proj"] is not None for c_ in cells)))
                   and self.bf16 and self.use_shadows and not residual and not ps.use_bn and not ps.layer_norm and P % 4 == 0
                   else None)
            for d, c in enumerate(cells):
                half = Y[:, d * P:(d + 1) * P]
                if c["proj"] is not None:
                    ep = None
                    if drop and self.fuse_dropout:          # ... and that pass is the projection's own epilogue
                        # (shadow_only: the fp32 layer output stays unwritten where every reader - the next layer's zx product,
                        # its dKx, the head and its weight gradient - takes the bf16 shadow: _shadow_only)
                        ep = ops.Epilogue(self.keep, drop_seed, 2 * i + d, P,
                                          None if Y16 is None else Y16[:, d * P:(d + 1) * P],
                                          shadow_only=Y16 is not None and ps.E == 0 and self._shadow_only(rows, ndir * P))
                    elif not drop and Y16 is not None:      # no mask: the shadow alone (keep = 1 leaves the values as they are)
                        ep = ops.Epilogue(1.0, 0, 0, 1, Y16[:, d * P:(d + 1) * P],
                                          shadow_only=ps.E == 0 and self._shadow_only(rows, ndir * P))
                    self._mm(dirs[d]["hs"], c["proj"], out=half, epilogue=ep)        # m_t = m'_t . proj, batched
                elif drop and self.fuse_dropout:                                     # the strided copy carries the mask
                    ops.dropout_scale(dirs[d]["hs"], self.keep, drop_seed, 2 * i + d, out=half,
                                      shadow=None if Y16 is None else Y16[:, d * P:(d + 1) * P])
                else:
                    ops.dropout_scale(dirs[d]["hs"], 1.0, 0, 0, out=half)            # plain strided copy
            if ps.blstm:
                if drop:
                    for d, c in enumerate(cells):
                        if not self.fuse_dropout:
                            ops.dropout_scale(Y[:, d * P:(d + 1) * P], self.keep, drop_seed, 2 * i + d,
                                              shadow=None if Y16 is None else Y16[:, d * P:(d + 1) * P])
                if Y16 is not None:
                    self._adopt_shadow(Y, Y16)
                if residual:
                    ops.dropout_scale(inp, 1.0, 0, 0, out=Y, accumulate=True)        # finput + concat
            elif ps.cudnn:
                residual = False                                                     # bare cells (lstm.py:73-76)
            else:
                residual = not (i == 0 and D0 != P)                                  # lstm.py:236-260
                if residual:
                    ops.dropout_scale(inp, 1.0, 0, 0, out=Y, accumulate=True)        # ResidualWrapper
                    if ps.use_bn:         # a batch-normalised input is non-zero in the padded frames, but
                        ops.length_mask_(Y, seq_len, T, B)    # dynamic_rnn zeroes the wrapped cell's output there
                if self.keep < 1.0 and not ps.layer_norm:
                    ops.dropout_scale(Y, self.keep, drop_seed, 2 * i)
            layers.append(dict(inp=inp, inp_packed=inp_packed, dirs=dirs, cells=cells, Y=Y, residual=residual, T=T,
                               seq_len=seq_len, reduced=reduced))
            inp = batch_norm("drnn_bn%d" % i, Y) if ps.use_bn else Y                  # lstm.py:288-294
            if ps.layer_norm:
                # the next layer (and the top of the stack) reads dropout(LN(Y)): one pass, a fresh fp32 tensor in every
                # compute_dtype (the bf16 modes cast their own shadow of it); dead frames +0, like the plain model's Y
                inp = ops.layer_norm_fwd(Y, ps.p("ln%d/gamma" % i), ps.p("ln%d/beta" % i), seq_len, T, B, self.keep, drop_seed,
                                         2 * i, P if ps.blstm else ndir * P)
        pre_conv = None
        if self.row_conv:
            # lookahead: the head reads sum_j w[j] * top[t + j] over the live frames (fp32 in every compute_dtype; a fresh
            # tensor, so the head product casts its own shadow).  The batch-normalised top is non-zero in dead frames: the
            # pass never reads them.
            pre_conv, inp = inp, ops.row_conv_fwd(inp, ps.p("row_conv/kernel"), seq_len, T, B)
        head = {}
        if ps.E > 0:
            a = self._mm(inp, ps.p("Variable"), bias=ps.p("Variable_1"))
            q = self._mm(inp, ps.p("Variable_2"), bias=ps.p("Variable_3"))
            logits, pi = ops.moe_combine_fwd(a, q, ps.E, ps.V, self.tau, self.keep, drop_seed)
            head = dict(q=q, pi=pi)
        else:
            logits = self._mm(inp, ps.p("Variable"), bias=ps.p("Variable_1"))
        # (T and seq_len: the top layer's - what the head, the logits and encoder() are at; each layer keeps its own)
        self.saved = dict(layers=layers, head=head, T=T, B=B, seq_len=seq_len, drop_seed=drop_seed, bn=bn_saved,
                          top=inp, pre_conv=pre_conv, conv=conv_saved, frames=(pk_rows, pk_inverse) if self.packed else None,
                          chunks=(Tc, Bc, len_c) if chunked else None)
        return logits.view(T, B, ps.V)

    def encoder(self):
        """Final (c, m) states of the last layer, concatenated as bilstm.py:206-208.  Computed lazily
        from the saved activations (graph.py never uses it)."""
        if self.chunk:
            raise NotImplementedError("encoder(): with chunk_frames / lookahead_frames set the backward direction has one "
                                      "final state per chunk, not one per utterance")
        sv = self.saved
        B = sv["B"]
        last = sv["layers"][-1]
        sl = sv["seq_len"].long()
        outs = []
        for d, dd in enumerate(last["dirs"]):
            t_last = torch.zeros_like(sl) if dd["reverse"] else (sl - 1).clamp(min=0)
            idx = t_last * B + torch.arange(B, device=sl.device)
            # (bf16 mode may have left the fp32 hs unwritten: its shadow holds the values the projection reads anyway)
            h = (dd["hs_bf16"][idx].float() if dd.get("shadow_only") else dd["hs"][idx]).contiguous()
            proj = last["cells"][d]["proj"]
            outs += [dd["cs"][idx], self._mm(h, proj) if proj is not None else h]
        return torch.cat(outs, dim=1)

    # ------------------------------------------------------------------------------------ backward
    def layer_grad_range(self, i):
        """[lo, hi) of layer i's L2-decayed tensors (kernels, peepholes, projections of its cells) in the flat buffers."""
        ps = self.ps
        lo = ps.offsets[self._prefixes(i)[0] + "/kernel"]
        if i + 1 < ps.num_layers:
            hi = ps.offsets[self._prefixes(i + 1)[0] + "/kernel"]
        else:
            names = [s_[0] for s_ in ps.specs]
            k = max(j for j, nm in enumerate(names) if nm.startswith(self._prefixes(i)[-1] + "/") and "bias" not in nm)
            hi = ps.offsets[names[k + 1]] if k + 1 < len(names) else ps.n
        return lo, hi

    def backward(self, dlogits, buckets=None):
        """dlogits [T,B,V] -> fills ps.grad (overwrites; call once per forward).  ``buckets`` (dp.GradientBuckets, data
        parallelism): layer i + 1's gradient range is handed over once the BPTT of layer i is enqueued, and every
        outstanding bucket is waited for in front of the next recurrence."""
        ps, sv = self.ps, self.saved
        T, B = sv["T"], sv["B"]
        rows, N, P = T * B, ps.N, ps.Pout
        seed = sv["drop_seed"]
        dl = dlogits.reshape(rows, ps.V)
        ps.grad.zero_()
        top = sv["top"]
        keepalive = []
        packed = sv["frames"] is not None
        pk_rows, pk_inverse = sv["frames"] if packed else (None, None)

        def batch_norm_bwd(name, d):
            b = sv["bn"][name]
            return ops.bn_backward(b["x"], d, b["mean"], b["var"], ps.p(name + "/gamma"), self.is_training,
                                   ps.g(name + "/gamma"), ps.g(name + "/beta"), dx=d)


        # a BiLSTM layer 0 as wide as the convolutional front-end's output adds it to its own (bilstm.py:199): the one case in
        # which that residual carries a gradient - into the front-end
        front_residual = bool(self.conv) and ps.blstm and sv["layers"][0]["residual"]

        def masked_dY(i, width, across_reduction=False):
            """The epilogue that finishes layer i's dY inside the product writing it (the DropoutWrapper's backward: the
            forward mask again, per direction), plus the bf16 shadow both products of each half (dh, dproj) read -
            or (None, None) when layer i masks in a pass of its own."""
            if (not (self.fuse_dropout and ps.blstm and self.keep < 1.0 and not ps.use_bn and not ps.layer_norm) or packed
                    or across_reduction or (i == 0 and front_residual)):
                # (packed: the mask hashes the PADDED row index - it goes on the unpacked dY below; across a time reduction:
                # it hashes the index at layer i's own frame rate - it goes on the un-reduced dY; layer 0 adding the
                # front-end's output to its own: that residual branch takes the UNMASKED dY, so the mask goes on below)
                return None, None
            d16 = (torch.empty((rows, width), dtype=torch.bfloat16, device=dl.device)
                   if self.bf16 and self.use_shadows and P % 4 == 0 else None)
            # (shadow_only: dY is read through the shadow by both products of each half - dh = half . proj^T, dproj = hs^T half)
            return ops.Epilogue(self.keep, seed, 2 * i, P, d16,
                                shadow_only=d16 is not None and ps.E == 0 and self._shadow_only(rows, width)), d16

        ep, dY16 = masked_dY(ps.num_layers - 1, top.shape[1])
        premasked = ep is not None
        if ps.E > 0:
            q, pi = sv["head"]["q"], sv["head"]["pi"]
            da = ops.moe_combine_bwd(pi, q, dl, ps.E, ps.V, self.tau, self.keep, seed)       # q now holds dq
            dY = self._mm(da, ps.p("Variable"), tb=True)
            self._mm(q, ps.p("Variable_2"), tb=True, out=dY, beta=1.0, epilogue=ep)
            self._mm(top, da, ta=True, out=ps.g("Variable"))
            ops.colsum(da, out=ps.g("Variable_1"))
            self._mm(top, q, ta=True, out=ps.g("Variable_2"))
            ops.colsum(q, out=ps.g("Variable_3"))
        else:
            dY = self._mm(dl, ps.p("Variable"), tb=True, epilogue=ep)
            self._mm(top, dl, ta=True, out=ps.g("Variable"))
            ops.colsum(dl, out=ps.g("Variable_1"))
        if sv["pre_conv"] is not None:
            # the row convolution's backward: the filter's gradient, and dY becomes the gradient of the tensor it read
            dY, _ = ops.row_conv_bwd(sv["pre_conv"], dY, ps.p("row_conv/kernel"), sv["seq_len"], T, B,
                                     dw=ps.g("row_conv/kernel"))
        for i in reversed(range(ps.num_layers)):
            L = sv["layers"][i]
            cells, dirs, inp = L["cells"], L["dirs"], L["inp"]
            # this layer's own frame count, rows and lengths (all layers alike without time_reduce_layers)
            T, seq_len = L["T"], L["seq_len"]
            rows = T * B
            ndir = len(cells)
            need_dinp = i > 0 or ps.use_bn or bool(self.conv)
            dres = None
            if ps.use_bn:
                dY = batch_norm_bwd("drnn_bn%d" % i, dY)
            if ps.layer_norm:
                # dY becomes the gradient of the unmasked Y, in place (the pass applies the forward's mask to dY on load)
                ops.layer_norm_bwd(L["Y"], dY, ps.p("ln%d/gamma" % i), seq_len, T, B, self.keep, seed, 2 * i,
                                   P if ps.blstm else ndir * P, dx=dY, dgamma=ps.g("ln%d/gamma" % i),
                                   dbeta=ps.g("ln%d/beta" % i))
            if ps.blstm and i == 0 and front_residual:
                # Y_0 = dropout(concat) + front-end: its gradient is dY before the mask below (layer_norm: of the unmasked Y)
                dres = dY.clone() if self.keep < 1.0 and not ps.layer_norm else dY
            if ps.blstm:
                if premasked:                    # the product that wrote dY masked it and wrote its shadow
                    if dY16 is not None:
                        for d in range(ndir):
                            self._adopt_shadow(dY[:, d * P:(d + 1) * P], dY16[:, d * P:(d + 1) * P])
                elif self.keep < 1.0 and not ps.layer_norm:
                    dY16 = (torch.empty((rows, ndir * P), dtype=torch.bfloat16, device=dY.device)
                            if self.bf16 and self.use_shadows and P % 4 == 0 and dY.stride(0) % 4 == 0 else None)
                    for d in range(ndir):
                        half = dY[:, d * P:(d + 1) * P]
                        if dY16 is None:
                            ops.dropout_scale(half, self.keep, seed, 2 * i + d)
                        else:            # mask + the bf16 shadow both products of `half` (dh, dproj) read, one pass
                            ops.dropout_scale(half, self.keep, seed, 2 * i + d, shadow=dY16[:, d * P:(d + 1) * P])
                            self._adopt_shadow(half, dY16[:, d * P:(d + 1) * P])
            else:
                if self.keep < 1.0 and not ps.layer_norm:
                    ops.dropout_scale(dY, self.keep, seed, 2 * i)
                if L["residual"]:
                    if ps.use_bn:
                        ops.length_mask_(dY, sv["seq_len"], T, B)
                    dres = dY                                                            # d(out+inp)/d inp
            bdirs = []
            for d, c in enumerate(cells):
                half = dY[:, d * P:(d + 1) * P]
                if c["proj"] is not None:
                    dh = self._mm(half, c["proj"], tb=True)                              # [rows,N]
                    RT = ops.transpose(dirs[d]["R"])             # (proj.Kh)^T: the forward's fold, transposed (not redone)
                else:
                    dh = half.contiguous() if ndir > 1 else half
                    RT = ops.transpose(c["Kh"])
                # w_f_diag, w_i_diag, w_o_diag are adjacent in the flat gradient buffer: one [3,N] block
                dpeep = None
                if ps.peep:
                    o = ps.offsets[c["prefix"] + "/w_f_diag"]
                    dpeep = ps.grad[o:o + 3 * N]
                ck = dirs[d].get("chunked")
                if ck is not None:
                    # latency-controlled backward direction: its BPTT runs on the chunk rows; the outputs of lookahead
                    # frames were discarded, so their upstream gradient is zero (the state still carries gradient through them)
                    bdirs.append(dict(gates=ck["zx"], RT=RT, w_f=c["w_f"], w_i=c["w_i"], w_o=c["w_o"], cs=ck["cs"],
                                      dh=ops.chunk_gather(dh, T, B, self.chunk, self.lookahead, zero_lookahead=True),
                                      dpeep=dpeep, dbias=ps.g(c["prefix"] + "/bias"), reverse=True))
                    continue
                bdirs.append(dict(gates=dirs[d]["zx"], RT=RT, w_f=c["w_f"], w_i=c["w_i"], w_o=c["w_o"],
                                  cs=dirs[d]["cs"], dh=dh, dpeep=dpeep, dbias=ps.g(c["prefix"] + "/bias"),
                                  reverse=dirs[d]["reverse"]))
                if self.bf16 and self.use_shadows and (i > 0 or ps.use_bn or N % 256 == 0):
                    # dX = dz . Kx^T (and, in whole 256-tiles, dKx / dR on the K-major kernel) read dz as a bf16 shadow:
                    # written by the BPTT itself
                    bdirs[-1]["dz_bf16"] = torch.empty((rows, 4 * N), dtype=torch.bfloat16, device=dY.device)
                    bdirs[-1]["shadow_only"] = self._shadow_only(rows, c["I"])
                side_x3 = not (self.overlap_wgrad and i > 0 and self.x3_side_f32)      # this layer's weight gradients on x3?
                if self.x3_rec_bwd and N % 4 == 0 and (_x3_pays(rows, c["I"], 4 * N)
                                                or (side_x3 and _x3_pays(c["I"], 4 * N, rows, split_k=True))
                                                or (side_x3 and T > 1 and _x3_pays(N, 4 * N, rows - B, split_k=True))):
                    # the dX / dKx / dR products read dz as an x3 shadow: the split-operand BPTT's producers write it (they
                    # split dz for the exchange anyway); other schedules get the split pass behind the recurrence
                    bdirs[-1]["dz_x3"] = torch.empty((rows, 12 * N), dtype=torch.bfloat16, device=dY.device)
            if buckets is not None:
                buckets.wait()                   # a persistent recurrence needs every CU: no collective kernel beside it
            if sv["chunks"] is not None:
                # each direction in its own layout; dbias / dpeep of the chunked one accumulate over all chunk rows, which is
                # the right sum.  zx[t] was shared by every chunk copy of frame t: its gradient is the sum over the copies
                # (fixed order), and that padded dz takes the place of the recurrence's for dKx, dX and the packed path.
                # dz_c stays for dR, the one product in the chunk layout.
                Tc, Bc, len_c = sv["chunks"]
                ops.lstm_bwd(bdirs[:1], sv["seq_len"], T, B, N)
                ops.lstm_bwd(bdirs[1:], len_c, Tc, Bc, N)
                bdirs[1]["gates_c"] = bdirs[1]["gates"]
                bdirs[1]["gates"] = ops.chunk_fold(bdirs[1]["gates_c"], T, B, self.chunk, self.lookahead, sum_copies=True,
                                                   seq_len=sv["seq_len"])
            else:
                ops.lstm_bwd(bdirs, seq_len, T, B, N, bf16=self.bf16, x3=self.x3_rec_bwd)
            if buckets is not None and i + 1 < ps.num_layers and not self.overlap_wgrad:
                buckets.issue(*self.layer_grad_range(i + 1))      # runs beside this layer's weight-gradient GEMMs
            for bd in bdirs:
                if bd.get("dz_bf16") is not None:
                    self._adopt_shadow(bd["gates"], bd["dz_bf16"])
                if bd.get("dz_x3") is not None:
                    t_ = bd["gates"]
                    self._shadows[(t_.data_ptr(), tuple(t_.shape), t_.stride(0), False, "x3")] = (t_, bd["dz_x3"])
            # packed frames: dz's live rows, once per direction, for dKx and dX; dX is formed on packed rows and unpacked into
            # the padded dinp (dead rows zero - what dz = 0 there gives the padded product).  Packed on the main stream, in
            # front of the event the side stream waits for.
            dzp = [ops.pack_rows(bd["gates"], pk_rows) for bd in bdirs] if packed else None
            xin, dzs_in = (L["inp_packed"], dzp) if packed else (inp, [bd["gates"] for bd in bdirs])
            dinp = None
            if need_dinp and not packed:
                dinp = torch.empty((rows, inp.shape[1]), dtype=torch.float32, device=dY.device)
            # the buffer the dX products write: dinp itself, or its packed form
            dxo = torch.empty((pk_rows.shape[0], inp.shape[1]), dtype=torch.float32, device=dY.device) if need_dinp and packed else dinp
            # rides on the LAST product into dinp
            ep, next16 = masked_dY(i - 1, inp.shape[1], across_reduction=L["reduced"]) if i > 0 else (None, None)
            overlap = self.overlap_wgrad and i > 0
            side_x3 = not (overlap and self.x3_side_f32)
            # bf16 shadows, both directions: dinp = dz_f . Kx_f^T + dz_b . Kx_b^T as ONE product whose reduction walks both
            # operand pairs (lc_gemm_bf16_nt2) - dinp is written once instead of written, read back and written again
            fuse_dx = (self.bf16 and self.use_shadows and ndir == 2 and need_dinp and not overlap and N % 2 == 0
                       and self.fuse_dx)
            # ... and the same in float32 (lc_gemm_f32_nt2; not in bf16x3 mode, whose products are split-operand ones)
            fuse_dx32 = (not self.bf16 and not self.x3 and ndir == 2 and need_dinp and not overlap and self.fuse_dx
                         and dzs_in[0].stride(0) == dzs_in[1].stride(0)
                         and cells[0]["Kx"].stride(0) == cells[1]["Kx"].stride(0))
            if overlap and need_dinp:            # the next layer's BPTT waits for this only: issue it first
                # (the two-segment product here too was measured in round 6: c3 80.8 / 81.5 -> 80.7 / 81.5 ms, c2 inside its
                # run-to-run spread - not taken)
                for d, c in enumerate(cells):
                    self._mm(dzs_in[d], c["Kx"], tb=True, out=dxo, beta=(0.0 if d == 0 else 1.0),
                             epilogue=ep if d == ndir - 1 else None)
                if packed:
                    dinp = ops.unpack_rows(dxo, pk_inverse)
            main = torch.cuda.current_stream()
            if overlap:
                if self._side is None:
                    self._side = torch.cuda.Stream(device=dY.device, priority=0)
                ev = torch.cuda.Event()
                ev.record(main)
                self._side.wait_event(ev)
                # read on the side stream after main has dropped its references (dirs / bdirs: the chunked hs and dz too)
                keepalive.append((dY, bdirs, dzp, dirs))
            with torch.cuda.stream(self._side if overlap else main):
                for d, c in enumerate(cells):
                    pre = c["prefix"]
                    dz, hs = bdirs[d]["gates"], dirs[d]["hs"]
                    gk = ps.g(pre + "/kernel")
                    I = c["I"]
                    self._mm(xin, dzs_in[d], ta=True, out=gk[:I], x3_ok=side_x3)             # dKx = X^T dZ
                    steps = T
                    dz_c = bdirs[d].get("gates_c")
                    if dz_c is not None:         # chunked direction: the recurrence's own rows, one chunk step apart
                        steps = sv["chunks"][0]
                    if steps > 1:                                                            # dR = M'_{prev}^T dZ
                        if dz_c is not None:
                            Bc = sv["chunks"][1]
                            hprev, dzs = dirs[d]["chunked"]["hs"][Bc:], dz_c[:steps * Bc - Bc]
                        elif dirs[d]["reverse"]:
                            hprev, dzs = hs[B:], dz[:rows - B]
                        else:
                            hprev, dzs = hs[:rows - B], dz[B:]
                        dR_out = None if c["proj"] is not None else gk[I:]
                        if self.x3 and side_x3 and _x3_pays(N, 4 * N, rows - B, split_k=True):
                            # row windows, one step apart, of the x3 shadows of the WHOLE hs / dz (shared with the
                            # projection, dKx, dproj and dX)
                            hs_3, dz_3 = self._shadow3(hs), self._shadow3(dz)
                            if dirs[d]["reverse"]:
                                a_v, b_v = hs_3[B:rows], dz_3[:rows - B]
                            else:
                                a_v, b_v = hs_3[:rows - B], dz_3[B:rows]
                            dR = ops.gemm_bf16x3_tn(a_v, b_v, N, 4 * N, out=dR_out)
                        elif self.use_shadows and N % 256 == 0:
                            # row windows, one step apart, of the natural shadows of the WHOLE hs / dz (shared with dKx,
                            # dproj, dX and the projection): K-major kernel, nothing transposed
                            hs_n, dz_n = self._shadow(hs, tr=False), self._shadow(dz, tr=False)
                            if dirs[d]["reverse"]:
                                a_v, b_v = hs_n[B:rows], dz_n[:rows - B]
                            else:
                                a_v, b_v = hs_n[:rows - B], dz_n[B:rows]
                            dR = ops.gemm_bf16_tn(a_v, b_v, out=dR_out)
                        elif self.use_shadows and B % 8 == 0:
                            # column windows of the transposed shadows of the WHOLE hs / dz (shared with dKx, dproj)
                            hs_t, dz_t = self._shadow(hs, tr=True), self._shadow(dz, tr=True)
                            if dirs[d]["reverse"]:
                                a_v, b_v = hs_t[:, B:rows], dz_t[:, :rows - B]
                            else:
                                a_v, b_v = hs_t[:, :rows - B], dz_t[:, B:rows]
                            dR = ops.gemm_bf16_nt(a_v, b_v, out=dR_out, K=rows - B)
                        else:
                            dR = self._mm(hprev, dzs, ta=True, out=dR_out, x3_ok=side_x3)
                        if c["proj"] is not None:
                            ops.gemm(c["proj"], dR, ta=True, out=gk[I:])                     # dKh = proj^T dR
                    half = dY[:, d * P:(d + 1) * P]
                    if c["proj"] is not None:
                        gp = ps.g(pre + "/projection/kernel")
                        self._mm(hs, half, ta=True, out=gp, x3_ok=side_x3)                   # from m_t = m'_t.proj
                        if steps > 1:
                            ops.gemm(dR, c["Kh"], tb=True, out=gp, beta=1.0)                 # from R = proj.Kh
                    if need_dinp and not overlap and not fuse_dx and not fuse_dx32:
                        self._mm(dzs_in[d], c["Kx"], tb=True, out=dxo, beta=(0.0 if d == 0 else 1.0),
                                 epilogue=ep if d == ndir - 1 else None)
                if fuse_dx32:
                    ops.gemm_nt2(dzs_in[0], cells[0]["Kx"], dzs_in[1], cells[1]["Kx"], out=dxo, epilogue=ep)
                if packed and need_dinp and not overlap:
                    dinp = ops.unpack_rows(dxo, pk_inverse)
                if fuse_dx:
                    ops.gemm_bf16_nt2(self._shadow(bdirs[0]["gates"], tr=False), self._shadow(cells[0]["Kx"], tr=False),
                                      self._shadow(bdirs[1]["gates"], tr=False), self._shadow(cells[1]["Kx"], tr=False),
                                      out=dinp, epilogue=ep)
            if need_dinp:
                if dres is not None:
                    ops.dropout_scale(dres, 1.0, 0, 0, out=dinp, accumulate=True)
                if L["reduced"]:
                    # dinp is [rows, r * 2P] at this layer's rate: each frame's r parts go back to the frames of the layer
                    # below they came from (its dead frames +0); that layer masks its dY in a pass of its own, at its own rate
                    below = sv["layers"][i - 1]
                    dinp = ops.time_reduce_bwd(dinp, below["seq_len"], below["T"], B, self.time_reduce_factor)
                dY, dY16, premasked = dinp, next16, ep is not None
        if ps.use_bn:
            batch_norm_bwd("drnn_bn_0_0", dY)
        # the front-end, from its top layer down: dY is layer 0's dX (its dead frames are never read); the first layer has
        # nobody to hand a dx to
        L0 = sv["layers"][0]
        for k in reversed(range(len(self.conv))):
            c = sv["conv"][k]
            dY, _, _ = ops.conv_bwd(c["x"], c["y"], dY, ps.p("conv%d/kernel" % k), L0["seq_len"], L0["T"], B, c["F"],
                                    group_major=c["group_major"], want_dx=k > 0, dw=ps.g("conv%d/kernel" % k),
                                    dbias=ps.g("conv%d/bias" % k))
        if keepalive:
            torch.cuda.current_stream().wait_stream(self._side)     # gradients complete before anyone reads them
            keepalive.clear()
        self.saved = None
        self._shadows.clear()

    def update_moving_averages(self, bn_saved=None):
        """The batch-norm UPDATE_OPS the train op depends on (graph.py:194-196); call once per training step with the
        batch moments of that step's forward (default: the ones still saved, i.e. before backward())."""
        if bn_saved is None:
            bn_saved = (self.saved or {}).get("bn", {})
        for name, b in bn_saved.items():
            if self.is_training:
                ops.bn_update_moving(self.ps.aux[name + "/moving_mean"], self.ps.aux[name + "/moving_variance"],
                                     b["mean"], b["var"])
