"""Frame map of a ragged batch: which rows of the time-major ``[T*B, width]`` buffers are live frames.

The model's kernels work on ``T * B`` padded rows; with ``pack_frames`` the products that read a layer's INPUT (zx, dKx, dX)
run on a packed copy that holds the live frames only (``lc_pack_rows`` / ``lc_unpack_rows``).  The map
is host arithmetic on the utterance lengths (numpy, no GPU needed), uploaded once per distinct batch.
"""
import numpy as np

TILE = 256          # packed row counts are whole tiles of the big product kernels; the tail rows are zero rows


class FrameMap:
    """``FrameMap(seq_len_host, T, B)``: lengths in ANY order (no sorting, no permutation of the batch), clipped to [0, T].

    * ``M``        live frames, ``sum_b min(seq_len[b], T)``;  ``Mp = roundup(M, 256)``
    * ``rows``     int32 [Mp]: packed row -> padded row ``t * B + b``, enumerated TIME-MAJOR (t ascending, then b ascending,
                   over the live (t, b)), -1 for the tail.  In a length-sorted batch the live rows of step t are then one
                   contiguous run of the packed matrix - what a recurrence needs to read packed buffers directly.
    * ``inverse``  int32 [T * B]: padded row -> packed row, -1 for dead rows.
    """

    def __init__(self, seq_len_host, T, B):
        sl = np.asarray(seq_len_host).astype(np.int64).reshape(-1)
        if sl.shape[0] != B:
            raise ValueError("FrameMap: %d lengths for a batch of %d" % (sl.shape[0], B))
        T, B = int(T), int(B)
        self.T, self.B = T, B
        self.seq_len = np.clip(sl, 0, T).astype(np.int32)
        live = np.arange(T, dtype=np.int64)[:, None] < self.seq_len[None, :]          # [T, B]
        padded = np.flatnonzero(live.reshape(-1)).astype(np.int32)                    # ascending t * B + b: time-major
        self.M = int(padded.shape[0])
        self.Mp = (self.M + TILE - 1) // TILE * TILE
        self.rows = np.full(self.Mp, -1, np.int32)
        self.rows[:self.M] = padded
        self.inverse = np.full(T * B, -1, np.int32)
        self.inverse[padded] = np.arange(self.M, dtype=np.int32)
        self._device = None

    @property
    def full(self):
        """No dead frame: nothing to pack."""
        return self.M == self.T * self.B

    def step_run(self, t):
        """[lo, hi) of time step t's live rows in the packed matrix (one contiguous run, b ascending)."""
        lo = int((np.minimum(self.seq_len, t)).sum())
        return lo, lo + int((self.seq_len > t).sum())

    def device(self, device):
        """(rows, inverse) as int32 tensors on ``device``: uploaded once, kept with the map."""
        import torch
        device = torch.device(device)
        if self._device is None or self._device[0] != device:
            self._device = (device, torch.from_numpy(self.rows).to(device), torch.from_numpy(self.inverse).to(device))
        return self._device[1], self._device[2]
