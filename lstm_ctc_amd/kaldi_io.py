"""Kaldi binary float-matrix table writer — the one piece of the reference's pyKaldiIO that the hot path's
output side needs (``pyKaldiIO.BaseFloatMatrixWriter`` as used by bin/nnet-forward.py:30-31,96,113).

Binary matrix entry (pyKaldiIO/kaldi_table.py:950-975, kaldi_matrix.py:280-287, io_funcs.py:86-100,231-254):
    ``<key> `` ``\\0B`` ``FM `` ``\\x04`` int32 rows ``\\x04`` int32 cols, then rows*cols float32, row-major.
Supported wspecifiers: ``ark:-``, ``ark:<file>``, ``ark,scp:<ark>,<scp>`` and the ``t`` (text) option.
"""
import struct
import sys

import numpy as np


class BaseFloatMatrixWriter:
    def __init__(self, wspecifier):
        spec, _, target = wspecifier.partition(":")
        opts = [o.strip() for o in spec.split(",")]
        if "ark" not in opts:
            raise ValueError("unsupported wspecifier (need ark): %s" % wspecifier)
        self.text = "t" in opts
        self.scp = None
        ark_path = target
        if "scp" in opts:
            first, second = [t.strip() for t in target.split(",")]
            ark_path, scp_path = (first, second) if opts.index("ark") < opts.index("scp") else (second, first)
            self.scp = open(scp_path, "w")
        self.ark_path = ark_path
        self.close_ark = ark_path != "-"
        self.ark = sys.stdout.buffer if ark_path == "-" else open(ark_path, "wb")

    def Write(self, key, matrix):
        m = np.ascontiguousarray(matrix, dtype=np.float32)
        assert m.ndim == 2
        self.ark.write((key + " ").encode())
        if self.scp is not None:
            self.scp.write("%s %s:%d\n" % (key, self.ark_path, self.ark.tell()))
        if self.text:                                 # kaldi_matrix.py:289-298: ' [' + rows of '%f ' + ']'
            if m.shape[0] == 0 or m.shape[1] == 0:
                self.ark.write(b" []\n")
            else:
                body = "".join("\n  " + "".join("%f " % v for v in row) for row in m.tolist())
                self.ark.write((" [" + body + "]\n").encode())
        else:
            self.ark.write(b"\0B" + b"FM " + b"\x04" + struct.pack("<i", m.shape[0]) + b"\x04" +
                           struct.pack("<i", m.shape[1]))
            self.ark.write(m.astype("<f4").tobytes())
        return True

    def Close(self):
        self.ark.flush()
        if self.close_ark:
            self.ark.close()
        if self.scp is not None:
            self.scp.close()


def read_float_matrix_ark(path):
    """Minimal reader of the binary entries written above (tests / round trips)."""
    out = {}
    with open(path, "rb") as f:
        data = f.read()
    pos = 0
    while pos < len(data):
        sp = data.index(b" ", pos)
        key = data[pos:sp].decode()
        pos = sp + 1
        assert data[pos:pos + 5] == b"\0BFM ", data[pos:pos + 5]
        pos += 5
        assert data[pos] == 4
        rows = struct.unpack("<i", data[pos + 1:pos + 5])[0]
        assert data[pos + 5] == 4
        cols = struct.unpack("<i", data[pos + 6:pos + 10])[0]
        pos += 10
        out[key] = np.frombuffer(data[pos:pos + 4 * rows * cols], "<f4").reshape(rows, cols).copy()
        pos += 4 * rows * cols
    return out


class Int32VectorWriter(BaseFloatMatrixWriter):
    """Kaldi integer-vector table writer (what ``ali-to-phones`` / ``copy-int-vector`` read); wspecifiers as for
    :class:`BaseFloatMatrixWriter`.  Binary entry (Kaldi's BasicVectorHolder<int32>): ``<key> `` ``\\0B`` one byte
    ``\\x04`` (the size of the count) int32 count, then count little-endian int32 values as one block.  Text entry:
    ``<key> v0 v1 ... \\n``."""

    def Write(self, key, vector):
        v = np.ascontiguousarray(vector, dtype=np.int32).reshape(-1)
        self.ark.write((key + " ").encode())
        if self.scp is not None:
            self.scp.write("%s %s:%d\n" % (key, self.ark_path, self.ark.tell()))
        if self.text:
            self.ark.write(("".join("%d " % x for x in v.tolist()) + "\n").encode())
        else:
            self.ark.write(b"\0B" + b"\x04" + struct.pack("<i", v.size))
            self.ark.write(v.astype("<i4").tobytes())
        return True


def read_int32_vector_ark(path, text=False):
    """Minimal reader of the entries :class:`Int32VectorWriter` writes (tests / round trips): {key: int32 array}, in file
    order."""
    out = {}
    with open(path, "rb") as f:
        data = f.read()
    if text:
        for line in data.decode().splitlines():
            key, _, rest = line.partition(" ")
            out[key] = np.asarray([int(x) for x in rest.split()], np.int32)
        return out
    pos = 0
    while pos < len(data):
        sp = data.index(b" ", pos)
        key = data[pos:sp].decode()
        pos = sp + 1
        assert data[pos:pos + 3] == b"\0B\x04", data[pos:pos + 3]
        n = struct.unpack("<i", data[pos + 3:pos + 7])[0]
        pos += 7
        out[key] = np.frombuffer(data[pos:pos + 4 * n], "<i4").copy()
        pos += 4 * n
    return out


class FloatMatrixTable:
    """Lazy reader of a float-matrix ark as :class:`BaseFloatMatrixWriter` writes it: ``{key: matrix}`` without holding
    the matrices (a corpus' posteriors are tens of GB).  Opening makes ONE pass over a binary ark that reads the headers and
    seeks over the bodies, building ``{key: (offset, rows, cols)}``; :meth:`get` then reads one matrix with ``os.pread``
    (no shared file position: safe from several threads).  A text ark (``text=True``, what ``ark,t:`` writes) is parsed
    eagerly behind the same interface.  Raises ``ValueError`` / ``OSError`` for a file that is not such an ark."""

    def __init__(self, path, text=False):
        import os
        self.path, self.text = path, bool(text)
        self._index, self._eager, self._fd = {}, None, None
        if self.text:
            self._eager = {}
            with open(path, "r") as f:
                self._parse_text(f.read())
            return
        size = os.path.getsize(path)
        with open(path, "rb", buffering=0) as f:
            pos = 0
            while pos < size:
                # "<key> " + 15 header bytes.  With n bytes read and no blank among them the header ends at byte n + 16 or
                # later, so 16 more can be read without touching a body; bodies are sought over, never read.
                f.seek(pos)
                head = f.read(17)
                sp = head.find(b" ")
                while sp < 0:
                    more = f.read(16)
                    if not more:
                        raise ValueError("%s: no key at byte %d" % (path, pos))
                    head += more
                    sp = head.find(b" ")
                if sp == 0:
                    raise ValueError("%s: empty key at byte %d" % (path, pos))
                if len(head) < sp + 16:
                    head += f.read(sp + 16 - len(head))
                h = head[sp + 1:sp + 16]
                if len(h) != 15 or h[:5] != b"\0BFM " or h[5] != 4 or h[10] != 4:
                    raise ValueError("%s: not a binary float-matrix entry at byte %d" % (path, pos + sp + 1))
                rows, cols = struct.unpack("<i", h[6:10])[0], struct.unpack("<i", h[11:15])[0]
                if rows < 0 or cols < 0:
                    raise ValueError("%s: negative matrix shape at byte %d" % (path, pos + sp + 1))
                offset = pos + sp + 16
                self._index[head[:sp].decode()] = (offset, rows, cols)
                pos = offset + 4 * rows * cols         # a body cut short shows in get(), which reads it
        self._fd = os.open(path, os.O_RDONLY)

    def _parse_text(self, data):
        pos = 0
        while True:
            lb = data.find("[", pos)
            if lb < 0:
                if data[pos:].strip():
                    raise ValueError("%s: text after the last matrix" % self.path)
                return
            rb = data.find("]", lb)
            key = data[pos:lb].split()
            if rb < 0 or len(key) != 1:
                raise ValueError("%s: not a text float-matrix ark" % self.path)
            rows = [[float(x) for x in line.split()] for line in data[lb + 1:rb].splitlines() if line.strip()]
            if len(set(len(r) for r in rows)) > 1:
                raise ValueError("%s: ragged matrix \"%s\"" % (self.path, key[0]))
            self._eager[key[0]] = np.asarray(rows, np.float32).reshape(len(rows), len(rows[0]) if rows else 0)
            pos = rb + 1

    def __contains__(self, key):
        return key in (self._index if self._eager is None else self._eager)

    def __len__(self):
        return len(self._index if self._eager is None else self._eager)

    def keys(self):
        return (self._index if self._eager is None else self._eager).keys()

    def shape(self, key):
        if self._eager is not None:
            return self._eager[key].shape
        return self._index[key][1:]

    def get(self, key, default=None):
        """The matrix of ``key`` ([rows, cols] float32, the caller's own copy), or ``default``."""
        if self._eager is not None:
            m = self._eager.get(key)
            return default if m is None else m.copy()
        entry = self._index.get(key)
        if entry is None:
            return default
        import os
        offset, rows, cols = entry
        want, chunks = 4 * rows * cols, []
        while want:
            piece = os.pread(self._fd, want, offset)
            if not piece:
                raise OSError("%s: entry \"%s\" ends early" % (self.path, key))
            chunks.append(piece)
            offset += len(piece)
            want -= len(piece)
        return np.frombuffer(b"".join(chunks), "<f4").reshape(rows, cols).astype(np.float32)

    def __getitem__(self, key):
        m = self.get(key)
        if m is None:
            raise KeyError(key)
        return m

    def close(self):
        if self._fd is not None:
            import os
            os.close(self._fd)
            self._fd = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
