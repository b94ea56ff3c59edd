"""SpecAugment (Park et al., 2019: time and frequency masking of the filterbank input) - settings, the command-line form and
the numpy mirror of ``lc_spec_augment`` (include/lstm_ctc_hip.h).  No reference counterpart.

The device pass is ``ops.spec_augment``; ``mask_plan`` and ``apply_host`` here are its definition in numpy - what the tests
compare the kernel against bit for bit, and what ``report_spec_augment`` sums its shares with.  Pure host code: importing this
module touches neither torch nor the library.

Layout.  The loader splices ``left_context`` / ``right_context`` neighbours beside each frame and keeps every ``subsample``-th
row, so with s = max(subsample, 1) column c of row (t, b) belongs to spliced block i = c // base_dim, shows raw frame
u = clamp(t * s + i - l, 0, n - 1) with n = seq_len[b] * s, and bin f = (c % base_dim) % freq_bins (statics, deltas and double
deltas are feature groups of ``freq_bins`` bins each).  A time mask is an interval of RAW frames, a frequency mask an interval
of bins that holds in every feature group and every spliced block.
"""
import collections
import math

import numpy as np

STREAM = 0x53504543          # "SPEC": the stream id of the draws
MAX_MASKS = 8
PLAN_ROWS = 16               # rows 0-7 time masks, 8-15 frequency masks

Layout = collections.namedtuple("Layout", "base_dim left_context right_context subsample")


def layout_of(nnet_config):
    """The loader's layout as ``nnet_config`` states it (``input_dim`` is the width BEFORE splicing)."""
    return Layout(int(nnet_config["input_dim"]), int(nnet_config.get("left_context") or 0),
                  int(nnet_config.get("right_context") or 0), int(nnet_config.get("subsample") or 0))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class SpecAugment(object):
    """Immutable settings: ``time_masks`` masks of at most ``time_width`` raw frames each, and of at most ``time_percent``
    percent of the utterance; ``freq_masks`` masks of at most ``freq_width`` of the ``freq_bins`` bins of a feature group;
    masked elements become ``fill``.  Validates with ValueError."""
    __slots__ = ("time_masks", "time_width", "time_percent", "freq_masks", "freq_width", "freq_bins", "fill")

    def __init__(self, time_masks=0, time_width=0, time_percent=100, freq_masks=0, freq_width=0, freq_bins=None, fill=0.0):
        if freq_bins is None:
            raise ValueError("SpecAugment needs freq_bins (bins per feature group)")
        for name, v in (("time_masks", time_masks), ("time_width", time_width), ("time_percent", time_percent),
                        ("freq_masks", freq_masks), ("freq_width", freq_width), ("freq_bins", freq_bins)):
            if not _is_int(v):
                raise ValueError("SpecAugment: %s must be an int, got %r" % (name, v))
            if not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("SpecAugment: %s = %d does not fit 32 bits" % (name, v))
        for name, v in (("time_masks", time_masks), ("freq_masks", freq_masks)):
            if not 0 <= v <= MAX_MASKS:
                raise ValueError("SpecAugment: %s must lie in 0..%d, got %d" % (name, MAX_MASKS, v))
        for name, v in (("time_width", time_width), ("freq_width", freq_width)):
            if v < 0:
                raise ValueError("SpecAugment: %s must be >= 0, got %d" % (name, v))
        if not 0 <= time_percent <= 100:
            raise ValueError("SpecAugment: time_percent must lie in 0..100, got %d" % time_percent)
        if freq_bins <= 0:
            raise ValueError("SpecAugment: freq_bins must be > 0, got %d" % freq_bins)
        if freq_width > freq_bins:
            raise ValueError("SpecAugment: freq_width %d exceeds freq_bins %d" % (freq_width, freq_bins))
        if isinstance(fill, bool) or not isinstance(fill, (int, float, np.integer, np.floating)) or not math.isfinite(fill) \
                or abs(float(fill)) > float(np.finfo(np.float32).max):
            raise ValueError("SpecAugment: fill must be a finite float32 value, got %r" % (fill,))
        values = (int(time_masks), int(time_width), int(time_percent), int(freq_masks), int(freq_width), int(freq_bins),
                  float(np.float32(fill)))
        for name, v in zip(self.__slots__, values):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("SpecAugment is immutable")

    def __delattr__(self, name):
        raise AttributeError("SpecAugment is immutable")

    def _key(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, SpecAugment) and self._key() == other._key()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._key())

    def __str__(self):
        """The command-line form; ``parse_spec(str(spec)) == spec``."""
        return "time=%dx%d,freq=%dx%d,bins=%d,cap=%d,fill=%s" % (self.time_masks, self.time_width, self.freq_masks,
                                                                 self.freq_width, self.freq_bins, self.time_percent,
                                                                 repr(self.fill))

    def __repr__(self):
        return "SpecAugment(%s)" % ", ".join("%s=%r" % (n, getattr(self, n)) for n in self.__slots__)

    def check_layout(self, base_dim):
        if base_dim <= 0 or base_dim % self.freq_bins != 0:
            raise ValueError("SpecAugment: freq_bins %d does not divide input_dim %d" % (self.freq_bins, base_dim))


def parse_spec(text):
    """``time=2x40,freq=2x15,bins=40[,cap=20][,fill=0]`` -> SpecAugment: count x maximum width of the time masks (raw frames) and
    of the frequency masks (bins), bins per feature group, the cap on a time mask in percent of the utterance (default 100),
    the value written (default 0).  ``time`` and ``freq`` default to no masks; ``bins`` is required.  ValueError for anything
    else."""
    if not isinstance(text, str) or not text.strip():
        raise ValueError("spec-augment: empty value (want time=NxW,freq=NxW,bins=F[,cap=P][,fill=V])")
    seen = {}
    for item in text.split(","):
        key, sep, value = item.partition("=")
        key, value = key.strip(), value.strip()
        if not sep or not value:
            raise ValueError("spec-augment: \"%s\" is not key=value" % item)
        if key not in ("time", "freq", "bins", "cap", "fill"):
            raise ValueError("spec-augment: unknown key \"%s\" (time, freq, bins, cap, fill)" % key)
        if key in seen:
            raise ValueError("spec-augment: \"%s\" given twice" % key)
        seen[key] = value

    def integer(key, value):
        if not value.isdigit():                       # no signs, no spaces, no floats
            raise ValueError("spec-augment: %s wants non-negative integers, got \"%s\"" % (key, value))
        return int(value)

    def pair(key):
        if key not in seen:
            return 0, 0
        count, sep, width = seen[key].partition("x")
        if not sep:
            raise ValueError("spec-augment: %s wants COUNTxWIDTH, got \"%s\"" % (key, seen[key]))
        return integer(key, count), integer(key, width)

    if "bins" not in seen:
        raise ValueError("spec-augment: bins=F (bins per feature group) is required")
    (tm, tw), (fm, fw) = pair("time"), pair("freq")
    fill = 0.0
    if "fill" in seen:
        try:
            fill = float(seen["fill"])
        except ValueError:
            raise ValueError("spec-augment: fill wants a number, got \"%s\"" % seen["fill"])
    return SpecAugment(time_masks=tm, time_width=tw, time_percent=integer("cap", seen["cap"]) if "cap" in seen else 100,
                       freq_masks=fm, freq_width=fw, freq_bins=integer("bins", seen["bins"]), fill=fill)


# ----------------------------------------------------------------------------------------------------- the draws
def _fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def hash_u32(seed, stream, idx):
    """``lc_hash_u32`` (csrc/common.h): the 32-bit value ``lc_dropout_factor`` forms before its float conversion, for a 32-bit
    seed and stream id and 64-bit indices (any shape).  Returns uint32 of ``idx``'s shape."""
    idx = np.asarray(idx).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = (np.uint32(int(seed) & 0xFFFFFFFF) * np.uint32(0x9E3779B1)) ^ \
            (np.uint32(int(stream) & 0xFFFFFFFF) * np.uint32(0x85EBCA77) + np.uint32(0x165667B1))
        v = _fmix32((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ h)
        return _fmix32(v ^ ((idx >> np.uint64(32)).astype(np.uint32) + np.uint32(0x27D4EB2F)))


def _ranged(v, m):
    """(uint64(v) * m) >> 32 for uint32 v and int64 m >= 1 (arrays)."""
    with np.errstate(over="ignore"):
        return ((v.astype(np.uint64) * m.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def mask_plan(seed, seq_len, spec, subsample):
    """[B, 16, 2] int32 of (start, width): rows 0-7 the time masks of each utterance in raw frames, rows 8-15 its frequency
    masks in bins, unused rows (0, 0).  Bit-identical to the ``plan`` ``lc_spec_augment`` writes."""
    seq = np.asarray(seq_len).astype(np.int64).reshape(-1)
    B = seq.shape[0]
    s = max(int(subsample or 0), 1)
    n = np.maximum(seq, 0) * s
    k0 = np.arange(B, dtype=np.uint64) * np.uint64(32)
    draw = lambda k: hash_u32(seed, STREAM, k0 + np.uint64(k))
    plan = np.zeros((B, PLAN_ROWS, 2), np.int64)
    W = np.minimum(n * spec.time_percent // 100, spec.time_width)
    for j in range(spec.time_masks):
        w = _ranged(draw(2 * j), W + 1)
        plan[:, j, 0], plan[:, j, 1] = _ranged(draw(2 * j + 1), n - w + 1), w
    for j in range(spec.freq_masks):
        w = _ranged(draw(16 + 2 * j), np.full(B, spec.freq_width + 1, np.int64))
        plan[:, 8 + j, 0], plan[:, 8 + j, 1] = _ranged(draw(17 + 2 * j), spec.freq_bins - w + 1), w
    return plan.astype(np.int32)


def apply_host(x_tbd, seq_len, plan, spec, base_dim, left_context, right_context, subsample):
    """The pass itself on a time-major [T, B, D] float32 array, D = base_dim * (1 + left_context + right_context): a copy of
    ``x_tbd`` with ``spec.fill`` where a time mask of ``plan`` holds the element's raw frame or a frequency mask its bin, for the
    rows t < seq_len[b]; every other element bit for bit."""
    x = np.asarray(x_tbd)
    if x.dtype != np.float32 or x.ndim != 3:
        raise ValueError("apply_host: x must be float32 [T, B, D]")
    T, B, D = x.shape
    l, r, s = int(left_context or 0), int(right_context or 0), max(int(subsample or 0), 1)
    if D != base_dim * (1 + l + r):
        raise ValueError("apply_host: D = %d is not base_dim %d * (1 + %d + %d)" % (D, base_dim, l, r))
    spec.check_layout(base_dim)
    seq = np.asarray(seq_len).astype(np.int64).reshape(-1)
    plan = np.asarray(plan).astype(np.int64)
    out = x.copy()
    cols = np.arange(D)
    block, fbin = cols // base_dim, (cols % base_dim) % spec.freq_bins
    fill = np.float32(spec.fill)
    for b in range(B):
        live = int(min(max(seq[b], 0), T))
        if live == 0:
            continue
        n = int(seq[b]) * s
        u = np.clip(np.arange(live)[:, None] * s + np.arange(1 + l + r)[None, :] - l, 0, n - 1)          # [live, blocks]
        tmask = np.zeros(u.shape, bool)
        for t0, w in plan[b, :spec.time_masks]:
            tmask |= (u >= t0) & (u < t0 + w)
        fmask = np.zeros(spec.freq_bins, bool)
        for f0, w in plan[b, 8:8 + spec.freq_masks]:
            fmask[f0:f0 + w] = True
        mask = tmask[:, block] | fmask[fbin][None, :]
        out[:live, b][mask] = fill
    return out


def masked_shares(plan, seq_len, spec, subsample):
    """(raw frames under a time mask, live raw frames, bins under a frequency mask, bins) summed over a batch - overlaps
    counted once: what ``report_spec_augment`` adds up."""
    seq = np.maximum(np.asarray(seq_len).astype(np.int64).reshape(-1), 0)
    s = max(int(subsample or 0), 1)
    frames = masked_frames = masked_bins = 0
    for b in range(seq.shape[0]):
        n = int(seq[b]) * s
        hit = np.zeros(n, bool)
        for t0, w in plan[b, :spec.time_masks]:
            hit[t0:t0 + w] = True
        fhit = np.zeros(spec.freq_bins, bool)
        for f0, w in plan[b, 8:8 + spec.freq_masks]:
            fhit[f0:f0 + w] = True
        frames += n
        masked_frames += int(hit.sum())
        masked_bins += int(fhit.sum())
    return masked_frames, frames, masked_bins, int(seq.shape[0]) * spec.freq_bins
