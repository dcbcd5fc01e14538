"""Host-side mirror of the reference's operator surface for the hot path, over the C ABI.

`Reflexiv` exposes one method per Spark operator class of P/ReflexivMain.java (names kept),
taking and returning flat numpy arrays in the reference's record layout, plus the resident
device pipeline (`count_reads_dev`, `assemble_dev`) that keeps everything in HBM.  Every
method runs the HIP kernels; nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import time

import numpy as np

from . import _lib
from ._lib import Params, CRecords, RfxError, TWIN_DS, TWIN_RDD, RFX_OK, RFX_E_CAP  # noqa: F401


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _cap_error(where, need, detail) -> RfxError:
    """the RfxError of an RFX_E_CAP return; .need = the capacity the call reported (what to retry with)"""
    e = RfxError(RFX_E_CAP, where, detail)
    e.need = int(need)
    return e


@dataclass
class Records:
    """Flat SoA record set (include/reflexiv_hip.h rfx_records)."""
    key: np.ndarray
    marker: np.ndarray
    ext_off: np.ndarray
    ext: np.ndarray
    left: np.ndarray
    right: np.ndarray

    @property
    def n(self) -> int:
        return int(self.key.shape[0])

    @property
    def kw(self) -> int:
        """words per key: 1 (key is uint64[n]) or the second dimension of uint64[n, kw] (k > 32)"""
        return 1 if self.key.ndim == 1 else int(self.key.shape[1])

    def tuple_list(self):
        kk = [int(x) for x in self.key] if self.key.ndim == 1 else [tuple(int(x) for x in r) for r in self.key]
        return [(kk[i], int(self.marker[i]),
                 tuple(int(x) for x in self.ext[self.ext_off[i]:self.ext_off[i + 1]]),
                 int(self.left[i]), int(self.right[i])) for i in range(self.n)]

    def _c(self) -> CRecords:
        c = CRecords()
        c.n = self.n
        c.key, c.marker, c.ext_off = _p(self.key), _p(self.marker), _p(self.ext_off)
        c.ext, c.left, c.right = _p(self.ext), _p(self.left), _p(self.right)
        c.cap_n, c.cap_words = self.n, len(self.ext)
        c.key_words = self.kw
        return c

    @staticmethod
    def empty(cap_n: int, cap_words: int, kw: int = 1) -> "Records":
        cap_n, cap_words = max(1, cap_n), max(1, cap_words)
        key = np.empty(cap_n, np.uint64) if kw == 1 else np.empty((cap_n, kw), np.uint64)
        return Records(key, np.empty(cap_n, np.int32), np.empty(cap_n + 1, np.int64),
                       np.empty(cap_words, np.uint64), np.empty(cap_n, np.int32), np.empty(cap_n, np.int32))

    def _trim(self, c: CRecords) -> "Records":
        n = int(c.n)
        w = int(self.ext_off[n]) if n else 0
        return Records(self.key[:n].copy(), self.marker[:n].copy(), self.ext_off[:n + 1].copy(),
                       self.ext[:w].copy(), self.left[:n].copy(), self.right[:n].copy())


_DYN_CODE = np.full(256, 3, np.uint8)
_DYN_CODE[ord("A")], _DYN_CODE[ord("C")], _DYN_CODE[ord("G")] = 0, 1, 2      # nucleotideValue: A0 C1 G2, anything else 3
_DYN_NUC = np.frombuffer(b"ACGT", np.uint8)


@dataclass
class DynRecords:
    """The dynamic-k record set across the C ABI (rfx_dyn_records): keys and extensions as base codes with offsets."""
    key: np.ndarray        # uint8
    key_off: np.ndarray    # int64 [n+1]
    ext: np.ndarray        # uint8
    ext_off: np.ndarray    # int64 [n+1]
    marker: np.ndarray     # int32
    left: np.ndarray       # int32
    right: np.ndarray      # int32

    @property
    def n(self) -> int:
        return len(self.marker)

    def _c(self) -> "_lib.CDynRecords":
        c = _lib.CDynRecords()
        c.n = self.n
        c.key, c.key_off, c.ext, c.ext_off = (self.key.ctypes.data, self.key_off.ctypes.data, self.ext.ctypes.data, self.ext_off.ctypes.data)
        c.marker, c.left, c.right = self.marker.ctypes.data, self.left.ctypes.data, self.right.ctypes.data
        return c

    @staticmethod
    def empty(cap_n: int, cap_key: int, cap_ext: int) -> "DynRecords":
        return DynRecords(np.empty(max(1, cap_key), np.uint8), np.empty(cap_n + 1, np.int64), np.empty(max(1, cap_ext), np.uint8),
                          np.empty(cap_n + 1, np.int64), np.empty(max(1, cap_n), np.int32), np.empty(max(1, cap_n), np.int32),
                          np.empty(max(1, cap_n), np.int32))

    def _trim(self, c) -> "DynRecords":
        n = int(c.n)
        return DynRecords(self.key[:c.need_key].copy(), self.key_off[:n + 1].copy(), self.ext[:c.need_ext].copy(), self.ext_off[:n + 1].copy(),
                          self.marker[:n].copy(), self.left[:n].copy(), self.right[:n].copy())

    def rows(self):
        """the text rows DSBinarySubKmerWith{Short,Long}ExtensionToString write (FirstFour:226-263): (key, "m|l|r", extension)"""
        out = []
        for i in range(self.n):
            k = bytes(_DYN_NUC[self.key[self.key_off[i]:self.key_off[i + 1]]]).decode()
            e = bytes(_DYN_NUC[self.ext[self.ext_off[i]:self.ext_off[i + 1]]]).decode()
            out.append((k, f"{int(self.marker[i])}|{int(self.left[i])}|{int(self.right[i])}", e))
        return out

    @staticmethod
    def from_text(keys, exts, markers, lefts, rights) -> "DynRecords":
        ko = np.zeros(len(keys) + 1, np.int64); ko[1:] = np.cumsum([len(x) for x in keys])
        eo = np.zeros(len(exts) + 1, np.int64); eo[1:] = np.cumsum([len(x) for x in exts])
        kb = _DYN_CODE[np.frombuffer("".join(keys).encode(), np.uint8)] if ko[-1] else np.zeros(1, np.uint8)
        eb = _DYN_CODE[np.frombuffer("".join(exts).encode(), np.uint8)] if eo[-1] else np.zeros(1, np.uint8)
        cl = lambda v: max(-30000, min(30000, int(v)))             # buildingAlongFromThreeInt read back (FirstFour:2340-2366)
        return DynRecords(np.ascontiguousarray(kb), ko, np.ascontiguousarray(eb), eo, np.array(markers, np.int32),
                          np.array([cl(v) for v in lefts], np.int32), np.array([cl(v) for v in rights], np.int32))

    @staticmethod
    def from_kmer_rows(rows) -> "DynRecords":
        """DynamicKmerBinarizerFromReducedToSubKmer of FirstFour (:2931-3016): (k-mer text, "m|l|r") rows"""
        keys, exts, mk, lf, rt = [], [], [], [], []
        for kmer, attr in rows:
            kmer = kmer[1:] if kmer.startswith("(") else kmer
            a = (attr[:-1] if attr.endswith(")") else attr).split("|")
            keys.append(kmer[:-1]); exts.append(kmer[-1]); mk.append(1); lf.append(int(a[1])); rt.append(int(a[2]))
        return DynRecords.from_text(keys, exts, mk, lf, rt)

    @staticmethod
    def from_rows(rows) -> "DynRecords":
        """DynamicKmerBinarizerFromReducedToSubKmer of Iteration: (sub-k-mer text, "m|l|r", extension text) rows"""
        keys, exts, mk, lf, rt = [], [], [], [], []
        for k, attr, e in rows:
            k = k[1:] if k.startswith("(") else k
            a = (attr[:-1] if attr.endswith(")") else attr).split("|")
            keys.append(k); exts.append(e); mk.append(int(a[0])); lf.append(int(a[1])); rt.append(int(a[2]))
        return DynRecords.from_text(keys, exts, mk, lf, rt)


class DynPacked:
    """The packed dynamic-k record set (rfx_dyn_packed) over torch tensors in HBM: four key words per record and word-aligned
    extensions, 32 bases per word, first base in the two highest bits, every bit past the last base 0.  Capacities are the
    tensors' sizes; `n` is the number of records in use, the extension words in use are ext_off[n]."""
    FIELDS = ("key", "key_len", "ext", "ext_off", "ext_len", "marker", "left", "right")

    def __init__(self, cap_n: int, cap_words: int, device="cuda"):
        import torch
        self.cap_n, self.cap_words, self.n = int(cap_n), int(cap_words), 0
        m, w = max(1, self.cap_n), max(1, self.cap_words)
        self.key = torch.empty(m * 4, dtype=torch.int64, device=device)       # (uint64 words, held as int64 bit patterns)
        self.key_len = torch.empty(m, dtype=torch.uint8, device=device)
        self.ext = torch.empty(w, dtype=torch.int64, device=device)
        self.ext_off = torch.empty(self.cap_n + 1, dtype=torch.int64, device=device)   # (empty, not zeros: no kernel of torch's stream may
                                                                                      # still be pending when the library writes here)
        self.ext_len = torch.empty(m, dtype=torch.int32, device=device)
        self.marker = torch.empty(m, dtype=torch.int32, device=device)
        self.left = torch.empty(m, dtype=torch.int32, device=device)
        self.right = torch.empty(m, dtype=torch.int32, device=device)

    @property
    def words(self) -> int:
        """extension words in use (reads ext_off[n] back)"""
        return int(self.ext_off[self.n].item()) if self.n else 0

    def tensors(self):
        return [getattr(self, f) for f in self.FIELDS]

    def _c(self) -> "_lib.CDynPacked":
        c = _lib.CDynPacked()
        c.n = self.n
        for f in self.FIELDS:
            setattr(c, f, getattr(self, f).data_ptr())
        c.cap_n, c.cap_words, c.need_words = self.cap_n, self.cap_words, 0
        return c

    def _grown(self, co, device=None) -> "DynPacked":
        """after RFX_E_CAP: a set that holds what the call reported (co.n records, co.need_words words); this one where it already does"""
        if int(co.n) <= self.cap_n and int(co.need_words) <= self.cap_words:
            return self
        return DynPacked(max(self.cap_n, int(co.n)), max(self.cap_words, int(co.need_words)), device or self.key.device)

    def _take(self, co):
        self.n = int(co.n)

    def host(self):
        """the raw arrays in use, as numpy: (key [n, 4] uint64, key_len, ext uint64, ext_off, ext_len, marker, left, right)"""
        n = self.n
        w = self.words
        return (self.key[:4 * n].cpu().numpy().view(np.uint64).reshape(n, 4), self.key_len[:n].cpu().numpy(),
                self.ext[:w].cpu().numpy().view(np.uint64), self.ext_off[:n + 1].cpu().numpy(), self.ext_len[:n].cpu().numpy(),
                self.marker[:n].cpu().numpy(), self.left[:n].cpu().numpy(), self.right[:n].cpu().numpy())


class ContigsPacked:
    """The packed contig set of the de-duplication (rfx_contigs_packed) over torch tensors in HBM: 32 bases per word, the first base
    in the two highest bits, every contig on a word, every bit past its last base 0.  Capacities are the tensors' sizes; `n` is
    the number of contigs in use, the words in use are word_off[n]."""
    FIELDS = ("words_t", "word_off", "len")

    def __init__(self, cap_n: int, cap_words: int, device="cuda"):
        import torch
        self.cap_n, self.cap_words, self.n = int(cap_n), int(cap_words), 0
        self.words_t = torch.empty(max(1, self.cap_words), dtype=torch.int64, device=device)   # (uint64 words, held as int64 bit patterns)
        self.word_off = torch.empty(self.cap_n + 1, dtype=torch.int64, device=device)
        self.len = torch.empty(max(1, self.cap_n), dtype=torch.int64, device=device)

    @property
    def words(self) -> int:
        """words in use (reads word_off[n] back)"""
        return int(self.word_off[self.n].item()) if self.n else 0

    def tensors(self):
        return [getattr(self, f) for f in self.FIELDS]

    def _c(self) -> "_lib.CContigsPacked":
        c = _lib.CContigsPacked()
        c.n = self.n
        c.words, c.word_off, c.len = self.words_t.data_ptr(), self.word_off.data_ptr(), self.len.data_ptr()
        c.cap_n, c.cap_words, c.need_n, c.need_words = self.cap_n, self.cap_words, 0, 0
        return c

    def _grown(self, co, device=None) -> "ContigsPacked":
        """after RFX_E_CAP: a set that holds what the call reported (co.need_n contigs, co.need_words words)"""
        return ContigsPacked(max(self.cap_n, int(co.need_n)), max(self.cap_words, int(co.need_words)), device or self.word_off.device)

    def _take(self, co):
        self.n = int(co.n)

    def host(self):
        """the raw arrays in use, as numpy: (words uint64, word_off, len)"""
        n = self.n
        return (self.words_t[:self.words].cpu().numpy().view(np.uint64), self.word_off[:n + 1].cpu().numpy(), self.len[:n].cpu().numpy())


class EndextConsensus:
    """The two consensus sets of the end extension (rfx_endext_consensus) over torch tensors in HBM: `left` and `right` are
    ContigsPacked of one entry per input contig (left: from the base next to the contig outwards), `flags` int32 (1 = left flagged,
    2 = right flagged)."""

    def __init__(self, cap_n: int, cap_words_left: int = None, cap_words_right: int = None, device="cuda"):
        import torch
        self.left = ContigsPacked(cap_n, 10 * cap_n if cap_words_left is None else cap_words_left, device)
        self.right = ContigsPacked(cap_n, 10 * cap_n if cap_words_right is None else cap_words_right, device)
        self.flags = torch.empty(max(1, int(cap_n)), dtype=torch.int32, device=device)

    def _c(self) -> "_lib.CEndextConsensus":
        c = _lib.CEndextConsensus()
        c.left, c.right, c.flags = self.left._c(), self.right._c(), self.flags.data_ptr()
        return c

    def _grown(self, co, device=None) -> "EndextConsensus":
        """after RFX_E_CAP: sets that hold what the call reported; the words of the left and of the right set each on their own"""
        return EndextConsensus(max(self.left.cap_n, int(co.left.need_n)), max(self.left.cap_words, int(co.left.need_words)),
                               max(self.right.cap_words, int(co.right.need_words)), device or self.flags.device)

    def _take(self, co):
        self.left.n, self.right.n = int(co.left.n), int(co.right.n)


class EndextSet:
    """The contigs of 07EndExtend in output order (rfx_endext_set) over torch tensors in HBM: `set` is a ContigsPacked of BASES ONLY
    (reversed left consensus || contig || right consensus), the int32 arrays hold per contig the new left / right, the lengths the ID
    carries, the flags, the input contig and the new index."""
    ARRAYS = ("left", "right", "left_len", "right_len", "flags", "src_idx", "new_idx")

    def __init__(self, cap_n: int, cap_words: int, device="cuda"):
        import torch
        self.set = ContigsPacked(cap_n, cap_words, device)
        for a in self.ARRAYS:
            setattr(self, a, torch.empty(max(1, int(cap_n)), dtype=torch.int32, device=device))

    @property
    def n(self) -> int:
        return self.set.n

    def _c(self) -> "_lib.CEndextSet":
        c = _lib.CEndextSet()
        c.set = self.set._c()
        for a in self.ARRAYS:
            setattr(c, a, getattr(self, a).data_ptr())
        return c

    def _grown(self, co, device=None) -> "EndextSet":
        """after RFX_E_CAP: a set that holds what the call reported (co.set.need_n contigs, co.set.need_words words)"""
        return EndextSet(max(self.set.cap_n, int(co.set.need_n)), max(self.set.cap_words, int(co.set.need_words)), device or self.set.word_off.device)

    def _take(self, co):
        self.set.n = int(co.set.n)

    def host(self):
        """{array name: numpy int32 of the n entries in use}"""
        return {a: getattr(self, a)[:self.n].cpu().numpy() for a in self.ARRAYS}


class MapHits:
    """The rows of the end mapping (rfx_map_hits) over torch int32 tensors in HBM, one entry per row in row order: read index, target
    end number (2 contig + side), strand, offset (o at a left end, q at a right end) and v.  `n` rows are in use; `seed` is the seed
    of the call that wrote them."""
    ARRAYS = ("read", "end", "strand", "offset", "v")

    def __init__(self, cap_n: int, device="cuda"):
        import torch
        self.cap_n, self.n, self.seed = int(cap_n), 0, 0
        for a in self.ARRAYS:
            setattr(self, a, torch.empty(max(1, self.cap_n), dtype=torch.int32, device=device))

    def _c(self) -> "_lib.CMapHits":
        c = _lib.CMapHits()
        c.n, c.cap_n, c.need_n, c.seed = self.n, self.cap_n, 0, self.seed
        for a in self.ARRAYS:
            setattr(c, a, getattr(self, a).data_ptr())
        return c

    def _grown(self, co, device=None) -> "MapHits":
        """after RFX_E_CAP: room for the co.need_n rows the call reported, as it is"""
        return MapHits(int(co.need_n), device or self.read.device)

    def _take(self, co):
        self.n, self.seed = int(co.n), int(co.seed)

    def host(self):
        """{array name: numpy int32 of the n entries in use}"""
        return {a: getattr(self, a)[:self.n].cpu().numpy() for a in self.ARRAYS}


class MercyKmers:
    """The mercy k-mers of one call (rfx_dev_mercy_kmers) over a torch int64 tensor in HBM: the counter's key format (bit patterns of
    uint64, the last base in the lowest bits), in (read, position) order.  `n` of them are in use."""

    def __init__(self, cap_n: int, device="cuda"):
        import torch
        self.cap_n, self.n = int(cap_n), 0
        self.keys = torch.empty(max(1, self.cap_n), dtype=torch.int64, device=device)

    class _Call:
        """what one call takes and writes (the entry point has plain arguments, no struct): the array, its capacity, *out_n"""
        def __init__(self, keys: int, cap_n: int):
            self.keys, self.cap_n, self.n = keys, cap_n, C.c_int64(0)

    def _c(self) -> "MercyKmers._Call":
        return MercyKmers._Call(self.keys.data_ptr(), self.cap_n)

    def _grown(self, co, device=None) -> "MercyKmers":
        """after RFX_E_CAP: room for the co.n k-mers the call reported, as it is"""
        return MercyKmers(int(co.n.value), device or self.keys.device)

    def _take(self, co):
        self.n = int(co.n.value)

    def host(self):
        """numpy uint64 of the n keys in use"""
        return self.keys[:self.n].cpu().numpy().view(np.uint64)


def as_records(r) -> Records:
    """Accept any object with key/marker/ext_off/ext/left/right arrays (e.g. the oracle's Records)."""
    return Records(np.ascontiguousarray(r.key, np.uint64), np.ascontiguousarray(r.marker, np.int32),
                   np.ascontiguousarray(r.ext_off, np.int64), np.ascontiguousarray(r.ext, np.uint64),
                   np.ascontiguousarray(r.left, np.int32), np.ascontiguousarray(r.right, np.int32))


def sub_words(k: int) -> int:
    """words of a (k-1)-mer key (subKmerBinarySlots, U/DefaultParam.java:94): 1 up to k = 32"""
    return 1 if k <= 32 else (k - 2) // 31 + 1


def asm_words(k: int) -> int:
    """words of a k-mer in the assembler's 31-bases-per-word layout (kmerBinarySlotsAssemble, :85)"""
    return 1 if k <= 31 else (k - 1) // 31 + 1


def default_params(**kw) -> Params:
    p = Params()
    _lib.lib().rfx_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Reflexiv:
    """One context = one MI355X + one HIP stream."""

    def __init__(self, device: int = -1):
        self.L = _lib.lib()
        ctx = C.c_void_p()
        st = self.L.rfx_ctx_create(device, C.byref(ctx))
        if st != RFX_OK:
            raise RfxError(st, "rfx_ctx_create", "a gfx950 (MI355X) GPU is required; there is no CPU fallback")
        self.ctx = ctx

    def close(self):
        if getattr(self, "comm", None) and getattr(self, "ctx", None):
            self.comm_destroy()
        if getattr(self, "ctx", None):
            self.L.rfx_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st, where):
        if st != RFX_OK:
            raise RfxError(st, where, (self.L.rfx_last_error(self.ctx) or b"").decode())

    def use_stream(self, hip_stream: int):
        self._check(self.L.rfx_ctx_set_stream(self.ctx, C.c_void_p(hip_stream)), "rfx_ctx_set_stream")

    def sync(self):
        self._check(self.L.rfx_ctx_sync(self.ctx), "rfx_ctx_sync")

    # ------------------------------------------------ operators on host arrays

    def ReverseComplementKmerBinaryExtraction(self, bases, read_off, k=31, front_clip=0, end_clip=0):
        """P/ReflexivMain.java:3013-3075 -> canonical k-mers in read/window order."""
        bases = np.ascontiguousarray(bases, np.uint8)
        read_off = np.ascontiguousarray(read_off, np.int64)
        nr = len(read_off) - 1
        n = C.c_int64(0)
        st = self.L.rfx_extract_canon(self.ctx, _p(bases), _p(read_off), C.c_int64(nr), k, front_clip, end_clip,
                                      None, C.c_int64(0), C.byref(n))
        if st not in (RFX_OK, RFX_E_CAP):
            self._check(st, "rfx_extract_canon")
        out = np.empty(max(1, n.value), np.uint64)
        self._check(self.L.rfx_extract_canon(self.ctx, _p(bases), _p(read_off), C.c_int64(nr), k, front_clip,
                                             end_clip, _p(out), C.c_int64(n.value), C.byref(n)),
                    "rfx_extract_canon")
        return out[:n.value]

    def KmerCounting_and_CoverageFilter(self, kmers, min_cov=2, max_cov=10_000_000, twin=TWIN_DS):
        """reduceByKey(KmerCounting) + filter(KmerCoverageFilter), P/ReflexivMain.java:155-163."""
        kmers = np.ascontiguousarray(kmers, np.uint64)
        n = len(kmers)
        keys = np.empty(max(1, n), np.uint64)
        counts = np.empty(max(1, n), np.int32)
        m, d = C.c_int64(0), C.c_int64(0)
        self._check(self.L.rfx_count_filter(self.ctx, _p(kmers), C.c_int64(n), min_cov, max_cov, twin, _p(keys),
                                            _p(counts), C.c_int64(n), C.byref(m), C.byref(d)), "rfx_count_filter")
        return keys[:m.value].copy(), counts[:m.value].copy(), int(d.value)

    # k > 31: the counter's W = k//32+1 word k-mers (P/ReflexivDataFrameCounter64.java)
    def ReverseComplementKmerBinaryExtractionFromDataset64(self, bases, read_off, k=63, front_clip=0, end_clip=0):
        """:401-650 -> canonical k-mers uint64[n, W] in read/window order."""
        bases = np.ascontiguousarray(bases, np.uint8)
        read_off = np.ascontiguousarray(read_off, np.int64)
        nr = len(read_off) - 1
        W = k // 32 + 1
        n = C.c_int64(0)
        st = self.L.rfx_extract_canon_w(self.ctx, _p(bases), _p(read_off), C.c_int64(nr), k, front_clip, end_clip,
                                        None, C.c_int64(0), C.byref(n))
        if st not in (RFX_OK, RFX_E_CAP):
            self._check(st, "rfx_extract_canon_w")
        out = np.empty((max(1, n.value), W), np.uint64)
        self._check(self.L.rfx_extract_canon_w(self.ctx, _p(bases), _p(read_off), C.c_int64(nr), k, front_clip,
                                               end_clip, _p(out), C.c_int64(n.value), C.byref(n)),
                    "rfx_extract_canon_w")
        return out[:n.value]

    def groupBy_count_filter_w(self, kmers, k=63, min_cov=2, max_cov=10_000_000):
        """groupBy("kmerBlocks").count() + the two filters, :191-205 -> (keys[m, W], counts int64[m], n_distinct)."""
        W = k // 32 + 1
        kmers = np.ascontiguousarray(kmers, np.uint64).reshape(-1, W)
        n = len(kmers)
        keys = np.empty((max(1, n), W), np.uint64)
        counts = np.empty(max(1, n), np.int64)
        m, d = C.c_int64(0), C.c_int64(0)
        self._check(self.L.rfx_count_filter_w(self.ctx, _p(kmers), C.c_int64(n), k, min_cov, max_cov, _p(keys),
                                              _p(counts), C.c_int64(n), C.byref(m), C.byref(d)), "rfx_count_filter_w")
        return keys[:m.value].copy(), counts[:m.value].copy(), int(d.value)

    def kmers_per_read_w(self, read_len, k, front_clip=0, end_clip=0) -> int:
        return int(self.L.rfx_kmers_per_read_w(read_len, k, front_clip, end_clip))

    def count_reads_w_dev(self, d_words: int, n_reads: int, words_per_read: int, read_len: int, k: int,
                          d_out_keys: int, d_out_counts: int, cap: int, min_cov=2, max_cov=10_000_000,
                          front_clip=0, end_clip=0):
        """k > 31 twin of count_reads_dev -> (n_survivors, n_distinct, n_instances); keys cap*W words, counts int64."""
        n, d, inst = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_dev_count_reads_w(self.ctx, C.c_void_p(d_words), C.c_int64(n_reads), words_per_read, read_len,
                                          k, front_clip, end_clip, min_cov, max_cov, C.c_void_p(d_out_keys),
                                          C.c_void_p(d_out_counts), C.c_int64(cap), C.byref(n), C.byref(d),
                                          C.byref(inst))
        if st == RFX_E_CAP:
            raise _cap_error("rfx_dev_count_reads_w", n.value, f"needs room for {n.value} survivors, cap is {cap}")
        self._check(st, "rfx_dev_count_reads_w")
        return int(n.value), int(d.value), int(inst.value)

    def count_reads_ragged_w_dev(self, d_words: int, d_read_len: int, n_reads: int, words_per_read: int, max_read_len: int,
                                 k: int, d_out_keys: int, d_out_counts: int, cap: int, min_cov=2, max_cov=10_000_000,
                                 front_clip=0, end_clip=0):
        """count_reads_w_dev (k = 33..127, not a multiple of 32) for reads of different lengths (d_read_len: uint32 per read, as
        encode_reads_dev writes) -> (n_survivors, n_distinct, n_instances); keys cap*W words (W = k//32 + 1), counts int64,
        ascending."""
        n, d, inst = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_dev_count_reads_ragged_w(self.ctx, C.c_void_p(d_words), C.c_void_p(d_read_len), C.c_int64(n_reads),
                                                 words_per_read, max_read_len, k, front_clip, end_clip, min_cov, max_cov,
                                                 C.c_void_p(d_out_keys), C.c_void_p(d_out_counts), C.c_int64(cap),
                                                 C.byref(n), C.byref(d), C.byref(inst))
        if st == RFX_E_CAP:
            raise _cap_error("rfx_dev_count_reads_ragged_w", n.value, f"needs room for {n.value} survivors, cap is {cap}")
        self._check(st, "rfx_dev_count_reads_ragged_w")
        return int(n.value), int(d.value), int(inst.value)

    def KmerReverseComplement_and_ForwardSubKmerExtraction(self, keys, counts, k=31) -> Records:
        """k > 31 (DSKmerReverseComplement + DSForwardSubKmerExtraction of ReflexivDSMain64): keys uint64[n, (k-1)//31+1]
        in the assembler layout."""
        keys = np.ascontiguousarray(keys, np.uint64)
        counts = np.ascontiguousarray(counts, np.int32)
        n = len(counts)
        assert keys.size == n * asm_words(k), (keys.shape, k)
        out = Records.empty(2 * n, 2 * n, sub_words(k))
        c = out._c(); c.cap_n = 2 * n; c.cap_words = 2 * n
        self._check(self.L.rfx_rc_expand_subkmer(self.ctx, _p(keys), _p(counts), C.c_int64(n), k, C.byref(c)),
                    "rfx_rc_expand_subkmer")
        return out._trim(c)

    def sortByKey(self, r, P: int):
        """-> (sorted Records, part_start[P+1])."""
        r = as_records(r)
        out = Records.empty(r.n, len(r.ext), r.kw)
        ci, co = r._c(), out._c()
        co.cap_n, co.cap_words = r.n, len(r.ext)
        ps = np.empty(P + 1, np.int64)
        self._check(self.L.rfx_sort_records(self.ctx, C.byref(ci), P, C.byref(co), _p(ps)), "rfx_sort_records")
        return out._trim(co), ps

    def _fork(self, fn, name, r, part_start, k, min_error_cov, twin):
        r = as_records(r)
        part_start = np.ascontiguousarray(part_start, np.int64)
        P = len(part_start) - 1
        out = Records.empty(r.n, r.n, r.kw)
        ci, co = r._c(), out._c()
        co.cap_n, co.cap_words = r.n, r.n
        ops = np.empty(P + 1, np.int64)
        self._check(fn(self.ctx, C.byref(ci), _p(part_start), P, k, min_error_cov, twin, C.byref(co), _p(ops)), name)
        return out._trim(co), ops

    def FilterForkSubKmer(self, r, part_start, k=31, min_error_cov=8, twin=TWIN_DS):
        return self._fork(self.L.rfx_fork_filter_forward, "rfx_fork_filter_forward", r, part_start, k,
                          min_error_cov, twin)

    def FilterForkReflectedSubKmer(self, r, part_start, k=31, min_error_cov=8, twin=TWIN_DS):
        return self._fork(self.L.rfx_fork_filter_reflected, "rfx_fork_filter_reflected", r, part_start, k,
                          min_error_cov, twin)

    def ReflectedSubKmerExtractionFromForward(self, r, k=31) -> Records:
        r = as_records(r)
        out = Records.empty(r.n, r.n, r.kw)
        ci, co = r._c(), out._c()
        co.cap_n, co.cap_words = r.n, r.n
        self._check(self.L.rfx_reflect_from_forward(self.ctx, C.byref(ci), k, C.byref(co)),
                    "rfx_reflect_from_forward")
        return out._trim(co)

    def kmerRandomReflection(self, r, part_start, k=31) -> Records:
        r = as_records(r)
        part_start = np.ascontiguousarray(part_start, np.int64)
        out = Records.empty(r.n, r.n, r.kw)
        ci, co = r._c(), out._c()
        co.cap_n, co.cap_words = r.n, r.n
        self._check(self.L.rfx_random_reflection(self.ctx, C.byref(ci), _p(part_start), len(part_start) - 1, k,
                                                 C.byref(co)), "rfx_random_reflection")
        return out._trim(co)

    def ExtendReflexivKmer(self, r, part_start, k=31, twin=TWIN_DS, stage=2, scramble=2):
        """One extend pass (stage 0: ExtendReflexivKmer, 1: ...ToArrayFirstTime, 2: ...ToArrayLoop).
        scramble = 3: DSExtendReflexivKmerToArrayLoop of ReflexivDSMain64 after param.scramble went to 3
        (the task's emission marker starts at 1, :7484-7486)."""
        r = as_records(r)
        part_start = np.ascontiguousarray(part_start, np.int64)
        P = len(part_start) - 1
        out = Records.empty(r.n, len(r.ext), r.kw)
        ci, co = r._c(), out._c()
        co.cap_n, co.cap_words = r.n, len(r.ext)
        ops = np.empty(P + 1, np.int64)
        if scramble != 2:
            self._check(self.L.rfx_extend_pass_w(self.ctx, C.byref(ci), _p(part_start), P, k, stage, scramble,
                                                 C.byref(co), _p(ops)), "rfx_extend_pass_w")
        else:
            self._check(self.L.rfx_extend_pass(self.ctx, C.byref(ci), _p(part_start), P, k, twin, stage, C.byref(co),
                                               _p(ops)), "rfx_extend_pass")
        return out._trim(co), ops

    def extras_operator(self, op: int, r, part_start, k: int):
        """One operator class of the k > 31 from-counts extras (P/ReflexivDSMain64.java:584-619, 672-712): op 0
        DSReflexivAndForwardKmer, 1 DSFilterExtendableKmerPairs, 2 DSFilterUnExtendableKmer, 3 DSFilterStillExtendableKmerFromPairs,
        4 DSFilterStillExtendableKmerEnds, 5 / 6 DSFilterUnExtendableKmerLeftEnds / ...RightEnds -> (Records, out_part_start)"""
        r = as_records(r)
        part_start = np.ascontiguousarray(part_start, np.int64)
        P = len(part_start) - 1
        mul = 2 if op == 0 else 1
        out = Records.empty(mul * r.n, mul * len(r.ext), r.kw)
        ci, co = r._c(), out._c()
        co.cap_n, co.cap_words = mul * r.n, mul * len(r.ext)
        ops = np.empty(P + 1, np.int64)
        self._check(self.L.rfx_extras_operator(self.ctx, op, C.byref(ci), _p(part_start), P, k, C.byref(co), _p(ops)),
                    "rfx_extras_operator")
        return out._trim(co), ops

    def KmerToContig(self, r, k=31, min_contig=500, twin=TWIN_DS):
        r = as_records(r)
        ci = r._c()
        ln, nc = C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_contigs_text(self.ctx, C.byref(ci), k, min_contig, twin, None, C.c_int64(0), C.byref(ln),
                                     C.byref(nc))
        if st not in (RFX_OK, RFX_E_CAP):
            self._check(st, "rfx_contigs_text")
        buf = np.empty(max(1, ln.value), np.uint8)
        self._check(self.L.rfx_contigs_text(self.ctx, C.byref(ci), k, min_contig, twin, _p(buf),
                                            C.c_int64(ln.value), C.byref(ln), C.byref(nc)), "rfx_contigs_text")
        return bytes(buf[:ln.value]).decode(), int(nc.value)

    # ------------------------------------------------ resident device pipeline

    def encode_reads_dev(self, d_bases: int, d_read_off: int, n_reads: int, words_per_read: int, d_words: int,
                         d_read_len: int = 0):
        self._check(self.L.rfx_dev_encode_reads(self.ctx, C.c_void_p(d_bases), C.c_void_p(d_read_off),
                                                C.c_int64(n_reads), words_per_read, C.c_void_p(d_words),
                                                C.c_void_p(d_read_len) if d_read_len else None),
                    "rfx_dev_encode_reads")

    def kmers_per_read(self, read_len, k, front_clip=0, end_clip=0) -> int:
        return int(self.L.rfx_kmers_per_read(read_len, k, front_clip, end_clip))

    def count_reads_dev(self, d_words: int, n_reads: int, words_per_read: int, read_len: int, k: int,
                        d_out_keys: int, d_out_counts: int, cap: int, min_cov=2, max_cov=10_000_000,
                        twin=TWIN_DS, front_clip=0, end_clip=0):
        """extract + reduceByKey + filter from packed reads in HBM -> (n_survivors, n_distinct, n_instances)."""
        n, d, inst = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_dev_count_reads(self.ctx, C.c_void_p(d_words), C.c_int64(n_reads), words_per_read, read_len,
                                        k, front_clip, end_clip, min_cov, max_cov, twin, None, C.c_int64(0),
                                        C.c_void_p(d_out_keys), C.c_void_p(d_out_counts), C.c_int64(cap),
                                        C.byref(n), C.byref(d), C.byref(inst))
        if st == RFX_E_CAP:
            raise _cap_error("rfx_dev_count_reads", n.value, f"needs room for {n.value} survivors, cap is {cap}")
        self._check(st, "rfx_dev_count_reads")
        return int(n.value), int(d.value), int(inst.value)

    def count_reads_ragged_dev(self, d_words: int, d_read_len: int, n_reads: int, words_per_read: int, max_read_len: int,
                               k: int, d_out_keys: int, d_out_counts: int, cap: int, min_cov=2, max_cov=10_000_000,
                               twin=TWIN_DS, front_clip=0, end_clip=0):
        """count_reads_dev for reads of different lengths (d_read_len: uint32 per read, as encode_reads_dev writes)."""
        n, d, inst = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_dev_count_reads_ragged(self.ctx, C.c_void_p(d_words), C.c_void_p(d_read_len), C.c_int64(n_reads),
                                               words_per_read, max_read_len, k, front_clip, end_clip, min_cov, max_cov,
                                               twin, C.c_void_p(d_out_keys), C.c_void_p(d_out_counts), C.c_int64(cap),
                                               C.byref(n), C.byref(d), C.byref(inst))
        if st == RFX_E_CAP:
            raise _cap_error("rfx_dev_count_reads_ragged", n.value, f"needs room for {n.value} survivors, cap is {cap}")
        self._check(st, "rfx_dev_count_reads_ragged")
        return int(n.value), int(d.value), int(inst.value)

    def bucket_wide_by_owner_dev(self, d_words: int, n_reads: int, words_per_read: int, read_len: int, k: int,
                                 n_owners: int, d_out: int, cap_elems: int, d_owner_off: int, front_clip=0, end_clip=0):
        """k = 33..63: two-word k-mers (16 B each) grouped by owning rank -> owner_off[n_owners+1] (host)."""
        h = np.empty(n_owners + 1, np.int64)
        self._check(self.L.rfx_dev_bucket_wide_by_owner(self.ctx, C.c_void_p(d_words), C.c_int64(n_reads), words_per_read,
                                                        read_len, k, front_clip, end_clip, n_owners, C.c_void_p(d_out),
                                                        C.c_int64(cap_elems), C.c_void_p(d_owner_off), _p(h)),
                    "rfx_dev_bucket_wide_by_owner")
        return h

    def count_wide_elems_dev(self, d_elems: int, n_elems: int, k: int, d_out_keys: int, d_out_counts: int, cap: int,
                             min_cov=2, max_cov=10_000_000):
        m, d = C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_dev_count_wide_elems(self.ctx, C.c_void_p(d_elems), C.c_int64(n_elems), k, min_cov, max_cov,
                                             C.c_void_p(d_out_keys), C.c_void_p(d_out_counts), C.c_int64(cap),
                                             C.byref(m), C.byref(d))
        if st == RFX_E_CAP:
            raise _cap_error("rfx_dev_count_wide_elems", m.value, f"needs room for {m.value} survivors, cap is {cap}")
        self._check(st, "rfx_dev_count_wide_elems")
        return int(m.value), int(d.value)

    def count_kmers_dev(self, d_kmers: int, n: int, d_out_keys: int, d_out_counts: int, cap: int, min_cov=2,
                        max_cov=10_000_000, twin=TWIN_DS):
        m, d = C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_dev_count_kmers(self.ctx, C.c_void_p(d_kmers), C.c_int64(n), min_cov, max_cov, twin, None,
                                        C.c_int64(0), C.c_void_p(d_out_keys), C.c_void_p(d_out_counts),
                                        C.c_int64(cap), C.byref(m), C.byref(d))
        if st == RFX_E_CAP:
            raise _cap_error("rfx_dev_count_kmers", m.value, f"needs room for {m.value} survivors, cap is {cap}")
        self._check(st, "rfx_dev_count_kmers")
        return int(m.value), int(d.value)

    def bucket_by_owner_dev(self, d_words: int, n_reads: int, words_per_read: int, read_len: int, k: int,
                            n_owners: int, d_out: int, cap: int, d_owner_off: int, front_clip=0, end_clip=0):
        h = np.empty(n_owners + 1, np.int64)
        self._check(self.L.rfx_dev_bucket_by_owner(self.ctx, C.c_void_p(d_words), C.c_int64(n_reads), words_per_read,
                                                   read_len, k, front_clip, end_clip, n_owners, C.c_void_p(d_out),
                                                   C.c_int64(cap), C.c_void_p(d_owner_off), _p(h)),
                    "rfx_dev_bucket_by_owner")
        return h

    def bucket_records_by_owner_dev(self, d_words: int, n_reads: int, words_per_read: int, read_len: int, k: int,
                                    n_owners: int, d_out: int, cap_records: int, d_owner_off: int,
                                    front_clip=0, end_clip=0):
        """Super-k-mer records (16 B each) grouped by owning rank.  d_out = 0: only returns how many
        records there are.  -> (n_records, owner_off[n_owners+1] or None)"""
        h = np.empty(n_owners + 1, np.int64)
        nrec = C.c_int64(0)
        st = self.L.rfx_dev_bucket_records_by_owner(self.ctx, C.c_void_p(d_words), C.c_int64(n_reads), words_per_read,
                                                    read_len, k, front_clip, end_clip, n_owners,
                                                    C.c_void_p(d_out) if d_out else None, C.c_int64(cap_records),
                                                    C.c_void_p(d_owner_off), _p(h), C.byref(nrec))
        if st == RFX_E_CAP:
            return int(nrec.value), None
        self._check(st, "rfx_dev_bucket_records_by_owner")
        return int(nrec.value), h

    def count_records_dev(self, d_records: int, n_records: int, n_instances_hint: int, k: int, d_out_keys: int,
                          d_out_counts: int, cap: int, min_cov=2, max_cov=10_000_000, twin=TWIN_DS):
        m, d = C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_dev_count_records(self.ctx, C.c_void_p(d_records), C.c_int64(n_records),
                                          C.c_int64(n_instances_hint), k, min_cov, max_cov, twin,
                                          C.c_void_p(d_out_keys), C.c_void_p(d_out_counts), C.c_int64(cap),
                                          C.byref(m), C.byref(d))
        if st == RFX_E_CAP:
            raise _cap_error("rfx_dev_count_records", m.value, f"needs room for {m.value} survivors, cap is {cap}")
        self._check(st, "rfx_dev_count_records")
        return int(m.value), int(d.value)

    def bucket_wide_records_by_owner_dev(self, d_words: int, n_reads: int, wpr: int, read_len: int, k: int, n_owners: int,
                                         d_out_records: int, cap_records: int, d_owner_off: int, front_clip=0, end_clip=0):
        """k = 33..63: 32-byte super-k-mer records grouped by owner -> (n_records, owner_off host or None when the
        buffer is missing / short: n_records is then the capacity needed)."""
        nrec = C.c_int64(0)
        h = np.zeros(n_owners + 1, np.int64)
        st = self.L.rfx_dev_bucket_wide_records_by_owner(self.ctx, C.c_void_p(d_words), C.c_int64(n_reads), wpr, read_len, k,
                                                         front_clip, end_clip, n_owners, C.c_void_p(d_out_records),
                                                         C.c_int64(cap_records), C.c_void_p(d_owner_off), _p(h), C.byref(nrec))
        if st == RFX_E_CAP:
            return int(nrec.value), None
        self._check(st, "rfx_dev_bucket_wide_records_by_owner")
        return int(nrec.value), h

    def count_wide_records_dev(self, d_records: int, n_records: int, n_instances_hint: int, k: int, d_out_keys: int,
                               d_out_counts: int, cap: int, min_cov=2, max_cov=10_000_000):
        m, d = C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_dev_count_wide_records(self.ctx, C.c_void_p(d_records), C.c_int64(n_records),
                                               C.c_int64(n_instances_hint), k, min_cov, max_cov, C.c_void_p(d_out_keys),
                                               C.c_void_p(d_out_counts), C.c_int64(cap), C.byref(m), C.byref(d))
        if st == RFX_E_CAP:
            raise _cap_error("rfx_dev_count_wide_records", m.value, f"needs room for {m.value} survivors, cap is {cap}")
        self._check(st, "rfx_dev_count_wide_records")
        return int(m.value), int(d.value)

    # ---- the exchange after a local combine (reduceByKey's map-side combine, P/ReflexivMain.java:155)
    def combine_reads_dev(self, d_words: int, n_reads: int, wpr: int, read_len: int, k: int, n_owners: int,
                          d_scratch_pairs: int, d_out_pairs: int, cap_pairs: int, d_owner_off: int,
                          front_clip=0, end_clip=0):
        """reads -> every distinct canonical k-mer with its local count as 16-byte {k-mer, count} pairs grouped
        by owner (no filter) -> (n_pairs, owner_off host int64[n_owners+1], instances); RfxError(RFX_E_CAP)
        carries the capacity needed in `.need`."""
        m, inst = C.c_int64(0), C.c_int64(0)
        h = np.zeros(n_owners + 1, np.int64)
        st = self.L.rfx_dev_combine_reads(self.ctx, C.c_void_p(d_words), C.c_int64(n_reads), wpr, read_len, k,
                                          front_clip, end_clip, n_owners, C.c_void_p(d_scratch_pairs),
                                          C.c_void_p(d_out_pairs), C.c_int64(cap_pairs), C.c_void_p(d_owner_off), _p(h),
                                          C.byref(m), C.byref(inst))
        if st == RFX_E_CAP:
            e = RfxError(st, "rfx_dev_combine_reads", f"needs room for {m.value} pairs, cap is {cap_pairs}")
            e.need = int(m.value)
            raise e
        self._check(st, "rfx_dev_combine_reads")
        return int(m.value), h, int(inst.value)

    def bucket_pairs_by_owner_dev(self, d_pairs: int, n_pairs: int, n_owners: int, d_out_pairs: int, d_owner_off: int):
        h = np.zeros(n_owners + 1, np.int64)
        self._check(self.L.rfx_dev_bucket_pairs_by_owner(self.ctx, C.c_void_p(d_pairs), C.c_int64(n_pairs), n_owners,
                                                         C.c_void_p(d_out_pairs), C.c_void_p(d_owner_off), _p(h)),
                    "rfx_dev_bucket_pairs_by_owner")
        return h

    def merge_pairs_dev(self, d_pairs: int, n_pairs: int, k: int, d_out_keys: int, d_out_counts: int, cap: int,
                        min_cov=2, max_cov=10_000_000, twin=TWIN_DS):
        m, d = C.c_int64(0), C.c_int64(0)
        st = self.L.rfx_dev_merge_pairs(self.ctx, C.c_void_p(d_pairs), C.c_int64(n_pairs), k, min_cov, max_cov, twin,
                                        C.c_void_p(d_out_keys), C.c_void_p(d_out_counts), C.c_int64(cap),
                                        C.byref(m), C.byref(d))
        if st == RFX_E_CAP:
            raise _cap_error("rfx_dev_merge_pairs", m.value, f"needs room for {m.value} survivors, cap is {cap}")
        self._check(st, "rfx_dev_merge_pairs")
        return int(m.value), int(d.value)

    def _text_buffer(self, cap: int):
        """The contig text of the device-resident drivers lands in one host buffer that the object keeps (grow-only):
        a fresh multi-hundred-megabyte mapping per call costs its page faults on every megabyte the text touches."""
        buf = getattr(self, "_textbuf", None)
        if buf is None or len(buf) < cap:
            buf = self._textbuf = np.empty(cap, np.uint8)
        return buf, len(buf)

    def assemble_dev(self, d_keys: int, d_counts: int, n: int, prm: Params):
        """Driver P/ReflexivMain.java:168-310 from the filtered (kmer,count) list in HBM
        -> (contig text, n_contigs, trace)."""
        trace = np.zeros(prm.max_iter + 8, np.int64)
        ln, nc, ntr = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        buf, cap = self._text_buffer(4 * (n + 16) * (prm.k + 8) + 1024)
        self._check(self.L.rfx_dev_assemble(self.ctx, C.c_void_p(d_keys), C.c_void_p(d_counts), C.c_int64(n),
                                            C.byref(prm), _p(buf), C.c_int64(cap), C.byref(ln), C.byref(nc),
                                            _p(trace), C.c_int64(len(trace)), C.byref(ntr)), "rfx_dev_assemble")
        return str(memoryview(buf)[:ln.value], "ascii"), int(nc.value), [int(x) for x in trace[:ntr.value]]

    def order_kmers_w_dev(self, d_keys: int, d_counts: int, n: int, k: int):
        """k = 33..127, not 64 or 96: (W-word k-mer, int64 count) pairs in any order -> ascending k-mer order, in place."""
        self._check(self.L.rfx_dev_order_kmers_w(self.ctx, C.c_void_p(d_keys), C.c_void_p(d_counts), C.c_int64(n), k),
                    "rfx_dev_order_kmers_w")

    def counter_to_asm_dev(self, d_keys32: int, d_counts64: int, n: int, k: int, d_out_kmers: int, d_out_counts: int,
                           min_cov=2, max_cov=10_000_000) -> int:
        """KmerBinarizer + the from-counts filter (P/ReflexivDSMain64.java:10772-10836, :473-478) in HBM: the counter's
        (k//32+1)-word k-mers and int64 counts -> (k-1)//31+1 words of 31 bases and int32 counts -> kept."""
        m = C.c_int64(0)
        self._check(self.L.rfx_dev_counter_to_asm(self.ctx, C.c_void_p(d_keys32), C.c_void_p(d_counts64), C.c_int64(n), k,
                                                  min_cov, max_cov, C.c_void_p(d_out_kmers), C.c_void_p(d_out_counts),
                                                  C.byref(m)), "rfx_dev_counter_to_asm")
        return int(m.value)

    def assemble_w_dev(self, d_kmers: int, d_counts: int, n: int, prm: Params):
        """k > 31 driver ReflexivDSMain64.assemblyFromKmer (:458-826, without the extras of :584-619 / :672-712)
        from the filtered (k-mer, count) list in HBM (assembler layout) -> (contig text, n_contigs, trace)."""
        trace = np.zeros(prm.max_iter + 8, np.int64)
        ln, nc, ntr = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        buf, cap = self._text_buffer(4 * (n + 16) * (prm.k + 8) + 1024)
        self._check(self.L.rfx_dev_assemble_w(self.ctx, C.c_void_p(d_kmers), C.c_void_p(d_counts), C.c_int64(n),
                                              C.byref(prm), _p(buf), C.c_int64(cap), C.byref(ln), C.byref(nc),
                                              _p(trace), C.c_int64(len(trace)), C.byref(ntr)), "rfx_dev_assemble_w")
        return str(memoryview(buf)[:ln.value], "ascii"), int(nc.value), [int(x) for x in trace[:ntr.value]]

    def synth_genome_dev(self, seed: int, genome_len: int, d_genome: int):
        self._check(self.L.rfx_dev_synth_genome(self.ctx, C.c_uint64(seed), C.c_int64(genome_len),
                                                C.c_void_p(d_genome)), "rfx_dev_synth_genome")

    def synth_reads_dev(self, seed: int, d_genome: int, genome_len: int, first_read: int, n_reads: int,
                        read_len: int, words_per_read: int, d_words: int, err_per_2_32: int = 21474836):
        self._check(self.L.rfx_dev_synth_reads(self.ctx, C.c_uint64(seed), C.c_void_p(d_genome),
                                               C.c_int64(genome_len), C.c_int64(first_read), C.c_int64(n_reads),
                                               read_len, C.c_uint32(err_per_2_32), words_per_read,
                                               C.c_void_p(d_words)), "rfx_dev_synth_reads")

    def sort_pairs_dev(self, d_keys: int, d_vals: int, n: int, key_bits: int, d_tmp_keys: int, d_tmp_vals: int):
        self._check(self.L.rfx_dev_sort_pairs(self.ctx, C.c_void_p(d_keys), C.c_void_p(d_vals), C.c_int64(n),
                                              key_bits, C.c_void_p(d_tmp_keys), C.c_void_p(d_tmp_vals)),
                    "rfx_dev_sort_pairs")

    def assemble_reads_ptr(self, bases_ptr: int, n_bases: int, read_off, prm: Params):
        """rfx_assemble_reads: ASCII reads in HOST memory (any lengths; bases_ptr may be pinned memory) -> upload, 2-bit
        encode, count / filter, the driver -> (text, n_contigs, trace, kept).  k <= 31; k = 33..125 (not 64 or 96) as the reference's
        `counter -kmer K` then `run -kmerc ... -kmer K` (the k > 31 counter, KmerBinarizer + the count filter, the k > 31
        driver; kept = the k-mers handed to the driver)."""
        read_off = np.ascontiguousarray(read_off, np.int64)
        n_reads = len(read_off) - 1
        trace = np.zeros(prm.max_iter + 8, np.int64)
        ln, nc, ntr, kept = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        buf, cap = self._text_buffer(1 << 24)
        while True:
            st = self.L.rfx_assemble_reads(self.ctx, C.c_void_p(bases_ptr), _p(read_off), C.c_int64(n_reads), C.byref(prm), _p(buf),
                                           C.c_int64(cap), C.byref(ln), C.byref(nc), _p(trace), C.c_int64(len(trace)), C.byref(ntr),
                                           C.byref(kept))
            if st == RFX_E_CAP and ln.value > cap:
                buf, cap = self._text_buffer(int(ln.value))
                continue
            if st == RFX_E_CAP:
                raise _cap_error("rfx_assemble_reads", ln.value, f"needs room for {ln.value} bytes of text, cap is {cap}")
            self._check(st, "rfx_assemble_reads")
            return str(memoryview(buf)[:ln.value], "ascii"), int(nc.value), [int(x) for x in trace[:ntr.value]], int(kept.value)

    def assemble_reads(self, bases, read_off, prm: Params):
        bases = np.ascontiguousarray(bases, np.uint8)
        return self.assemble_reads_ptr(bases.ctypes.data, len(bases), read_off, prm)

    # ------------------------------------------------ f-2: the dynamic-k record format and passes
    def _dyn_call(self, fn, name, r: DynRecords, make_args, grow=1):
        cap_n = r.n * grow
        cap_b = (len(r.key) + len(r.ext)) * grow + 64
        while True:
            out = DynRecords.empty(cap_n, cap_b, cap_b)
            ci, co = r._c(), out._c()
            co.cap_n, co.cap_key, co.cap_ext = cap_n, cap_b, cap_b
            t0 = time.perf_counter()
            st = fn(self.ctx, C.byref(ci), *make_args(co))
            self.last_call_ms = (time.perf_counter() - t0) * 1e3    # inside the C ABI (the last attempt): what a C / Java host pays
            if st == RFX_E_CAP:
                cap_n = max(cap_n, int(co.n)); cap_b = max(cap_b, int(co.need_key), int(co.need_ext)) + 64
                continue
            self._check(st, name)
            return out._trim(co)

    def dyn_binarize(self, rows, form=None) -> DynRecords:
        """rfx_dyn_binarize: DynamicKmerBinarizerFromReducedToSubKmer ON THE DEVICE.  rows: tuples of text fields -- (k-mer, "m|l|r")
        (form 0, FirstFour) or (sub-k-mer, "m|l|r", extension) (form 1, Iteration); joined by ',' as the hand-over files hold them."""
        rows = list(rows)
        if form is None:
            form = 1 if rows and len(rows[0]) == 3 else 0
        lines = [",".join(f) for f in rows]
        off = np.zeros(len(lines) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in lines])
        text = "".join(lines).encode()
        cap_n, cap_b = len(lines), len(text) + 64
        out = DynRecords.empty(cap_n, cap_b, cap_b)
        co = out._c()
        co.cap_n, co.cap_key, co.cap_ext = cap_n, cap_b, cap_b
        st = self.L.rfx_dyn_binarize(self.ctx, text, _p(off), C.c_int64(len(lines)), form, C.byref(co))
        self._check(st, "rfx_dyn_binarize")
        return out._trim(co)

    def dyn_sort(self, r: DynRecords, P: int):
        """rfx_dyn_sort -> (sorted DynRecords, part_start[P+1])"""
        ps = np.empty(P + 1, np.int64)
        out = self._dyn_call(self.L.rfx_dyn_sort, "rfx_dyn_sort", r, lambda co: (P, C.byref(co), _p(ps)))
        return out, ps

    def dyn_random_reflection(self, r: DynRecords, part_start):
        part_start = np.ascontiguousarray(part_start, np.int64)
        return self._dyn_call(self.L.rfx_dyn_random_reflection, "rfx_dyn_random_reflection", r,
                              lambda co: (_p(part_start), len(part_start) - 1, C.byref(co)))

    def dyn_extend_pass(self, r: DynRecords, part_start, stage=0, start_iteration=5, start_marker=2):
        part_start = np.ascontiguousarray(part_start, np.int64)
        P = len(part_start) - 1
        ops = np.empty(P + 1, np.int64)
        out = self._dyn_call(self.L.rfx_dyn_extend_pass, "rfx_dyn_extend_pass", r,
                             lambda co: (_p(part_start), P, stage, start_iteration, start_marker, C.byref(co), _p(ops)))
        return out, ops

    def dyn_run(self, r: DynRecords, P=1, random_reflection=False, passes_first_four=0, start_iteration=1, end_iteration=0):
        """rfx_dyn_run (records resident in HBM between the operators) -> (DynRecords, [records after each pass])"""
        trace = np.zeros(256, np.int64)
        ntr = C.c_int64(0)
        out = self._dyn_call(self.L.rfx_dyn_run, "rfx_dyn_run", r,
                             lambda co: (P, int(random_reflection), passes_first_four, start_iteration, end_iteration, C.byref(co), _p(trace),
                                         C.c_int64(len(trace)), C.byref(ntr)))
        return out, [int(x) for x in trace[:ntr.value]]

    # ---- the same passes on a packed record set that stays in HBM (rfx_dev_dyn_*)
    def _grow_call(self, fn, name, out, args_of, device=None, on_cap=None):
        """one call fn(ctx, *args_of(co)) with a packed output -- a DynPacked, ContigsPacked, EndextConsensus, EndextSet, MapHits or MercyKmers --
        into `out` -> out.  On RFX_E_CAP `out` is replaced by what its class builds from the needs the call reported (out._grown: on
        `device`, or where `out` lives) and the call made again; on_cap(): whatever else the caller has to regrow first.  On success
        the class takes what it keeps from the C struct (out._take)."""
        while True:
            co = out._c()
            t0 = time.perf_counter()
            st = fn(self.ctx, *args_of(co))
            self.last_call_ms = (time.perf_counter() - t0) * 1e3    # inside the C ABI (the last attempt)
            if st == RFX_E_CAP:
                if on_cap:
                    on_cap()
                out = out._grown(co, device)
                continue
            self._check(st, name)
            out._take(co)
            return out

    def dyn_pack(self, r: DynRecords, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_dyn_pack: host base codes -> a packed set in HBM"""
        out = out or DynPacked(r.n, r.n + len(r.ext) // 32)
        ci = r._c()
        return self._grow_call(self.L.rfx_dev_dyn_pack, "rfx_dev_dyn_pack", out, lambda co: (C.byref(ci), C.byref(co)))

    def dyn_unpack(self, d: "DynPacked") -> DynRecords:
        """rfx_dev_dyn_unpack: a packed set -> host base codes"""
        cap_n, cap_k, cap_e = d.n, 124 * d.n + 64, 32 * d.words + 64
        ci = d._c()
        while True:
            out = DynRecords.empty(cap_n, cap_k, cap_e)
            co = out._c()
            co.cap_n, co.cap_key, co.cap_ext = cap_n, cap_k, cap_e
            t0 = time.perf_counter()
            st = self.L.rfx_dev_dyn_unpack(self.ctx, C.byref(ci), C.byref(co))
            self.last_call_ms = (time.perf_counter() - t0) * 1e3
            if st == RFX_E_CAP:
                cap_n, cap_k, cap_e = max(cap_n, int(co.n)), max(cap_k, int(co.need_key)), max(cap_e, int(co.need_ext))
                continue
            self._check(st, "rfx_dev_dyn_unpack")
            return out._trim(co)

    def dyn_binarize_dev(self, d_text, d_row_off, form: int, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_dyn_binarize: text (torch uint8 tensor in HBM) + row offsets (torch int64 tensor, n_rows + 1) -> a packed set"""
        n_rows = int(d_row_off.numel()) - 1
        out = out or DynPacked(n_rows, n_rows + int(d_text.numel()) // 32)
        return self._grow_call(self.L.rfx_dev_dyn_binarize, "rfx_dev_dyn_binarize", out,
                                  lambda co: (d_text.data_ptr(), d_row_off.data_ptr(), n_rows, form, C.byref(co)))

    def dyn_sort_dev(self, d: "DynPacked", P: int, out: "DynPacked" = None):
        """rfx_dev_dyn_sort -> (sorted DynPacked, part_start: torch int64 [P + 1] in HBM)"""
        import torch
        ps = torch.empty(max(P, 0) + 1, dtype=torch.int64, device=d.key.device)
        ci = d._c()
        out = self._grow_call(self.L.rfx_dev_dyn_sort, "rfx_dev_dyn_sort", out or DynPacked(d.n, d.words),
                                 lambda co: (C.byref(ci), P, C.byref(co), ps.data_ptr()))
        return out, ps

    def dyn_random_reflection_dev(self, d: "DynPacked", d_part_start, out: "DynPacked" = None) -> "DynPacked":
        ci = d._c()
        P = int(d_part_start.numel()) - 1
        return self._grow_call(self.L.rfx_dev_dyn_random_reflection, "rfx_dev_dyn_random_reflection", out or DynPacked(d.n, d.words),
                                  lambda co: (C.byref(ci), d_part_start.data_ptr(), P, C.byref(co)))

    def dyn_extend_pass_dev(self, d: "DynPacked", d_part_start, stage=0, start_iteration=5, start_marker=2, out: "DynPacked" = None):
        """rfx_dev_dyn_extend_pass -> (DynPacked, out_part_start: torch int64 [P + 1] in HBM)"""
        import torch
        ci = d._c()
        P = int(d_part_start.numel()) - 1
        ops = torch.empty(P + 1, dtype=torch.int64, device=d.key.device)
        out = self._grow_call(self.L.rfx_dev_dyn_extend_pass, "rfx_dev_dyn_extend_pass", out or DynPacked(d.n, d.words),
                                 lambda co: (C.byref(ci), d_part_start.data_ptr(), P, stage, start_iteration, start_marker, C.byref(co),
                                             ops.data_ptr()))
        return out, ops

    def dyn_run_dev(self, d: "DynPacked", P=1, random_reflection=False, passes_first_four=0, start_iteration=1, end_iteration=0,
                    out: "DynPacked" = None):
        """rfx_dev_dyn_run -> (DynPacked, [records after each pass])"""
        ci = d._c()
        trace = np.zeros(256, np.int64)
        ntr = C.c_int64(0)
        out = self._grow_call(self.L.rfx_dev_dyn_run, "rfx_dev_dyn_run", out or DynPacked(d.n, d.words),
                                 lambda co: (C.byref(ci), P, int(random_reflection), passes_first_four, start_iteration, end_iteration,
                                             C.byref(co), trace.ctypes.data, len(trace), C.addressof(ntr)))
        return out, [int(x) for x in trace[:ntr.value]]

    def _params(self, struct, default_fn, c_name, *args, **kw):
        """a parameter struct: the library's defaults for `args`, then **kw"""
        p = struct()
        default_fn(C.byref(p), *(int(a) for a in args))
        for a, b in kw.items():
            if a not in dict(p._fields_):
                raise TypeError(f"{c_name} has no field {a!r}")
            setattr(p, a, b)
        return p

    def _host_text_call(self, name, caps, call):
        """one host-text entry point with len(caps) output texts: call(outs, caps, lens) -> its status.  On RFX_E_CAP every buffer
        grows to the length the call reported and the call is made again -> the texts as bytes"""
        caps = list(caps)
        lens = [C.c_int64(0) for _ in caps]
        while True:
            outs = [np.empty(max(1, c), np.uint8) for c in caps]
            t0 = time.perf_counter()
            st = call(outs, caps, lens)
            self.last_call_ms = (time.perf_counter() - t0) * 1e3    # inside the C ABI (the last attempt)
            if st == RFX_E_CAP and any(ln.value > c for ln, c in zip(lens, caps)):
                caps = [max(c, ln.value) for ln, c in zip(lens, caps)]
                continue
            self._check(st, name)
            return [o[:ln.value].tobytes() for o, ln in zip(outs, lens)]

    def _dev_text_call(self, name, d_text, call):
        """one device-text entry point: call(d_text, ln) -> its status.  On RFX_E_CAP d_text is replaced by one of the length
        the call reported and the call is made again -> (d_text, the text's length)"""
        import torch
        ln = C.c_int64(0)
        while True:
            t0 = time.perf_counter()
            st = call(d_text, ln)
            self.last_call_ms = (time.perf_counter() - t0) * 1e3    # inside the C ABI (the last attempt)
            if st == RFX_E_CAP:
                d_text = torch.empty(ln.value, dtype=torch.uint8, device=d_text.device)
                continue
            self._check(st, name)
            return d_text, int(ln.value)

    def dyn_to_text_dev(self, d: "DynPacked", d_text=None):
        """rfx_dev_dyn_to_text -> (torch uint8 tensor in HBM holding the rows "SUBKMER,m|l|r,EXTENSION\\n", its length)"""
        import torch
        ci = d._c()
        if d_text is None:
            d_text = torch.empty(max(1, 160 * d.n + 32 * d.words + 64), dtype=torch.uint8, device=d.key.device)
        return self._dev_text_call("rfx_dev_dyn_to_text", d_text, lambda t, ln: self.L.rfx_dev_dyn_to_text(
            self.ctx, C.byref(ci), t.data_ptr(), int(t.numel()), C.addressof(ln)))

    def dyn_run_text(self, text: bytes, form: int, P=1, random_reflection=False, passes_first_four=0, start_iteration=1, end_iteration=0):
        """rfx_dyn_run_text: the rows of a hand-over file (bytes; one row per line, empty lines skipped) -> (the output rows as
        bytes, [records after each pass]); binarizer, passes and the text writer on the device, on the packed set"""
        text = bytes(text)
        buf = np.frombuffer(text, np.uint8)
        # the line scan: a row starts at every non-empty line and runs to the next one (the line ends and any empty lines behind
        # it are the row's tail, which the device parser drops)
        ends = np.flatnonzero(buf == 10)
        starts = np.concatenate([[0], ends + 1]).astype(np.int64)
        stops = np.concatenate([ends, [len(buf)]]).astype(np.int64)
        stops = stops - ((stops > starts) & (buf[np.maximum(stops - 1, 0)] == 13) if len(buf) else 0)
        starts = starts[stops > starts]
        n_rows = len(starts)
        off = np.concatenate([starts, [len(buf)]]).astype(np.int64)
        cap = len(buf) + 32 * n_rows + 64
        trace = np.zeros(256, np.int64)
        ntr = C.c_int64(0)
        out, = self._host_text_call("rfx_dyn_run_text", [cap], lambda o, c, ln: self.L.rfx_dyn_run_text(
            self.ctx, text, off.ctypes.data, n_rows, form, P, int(random_reflection), passes_first_four, start_iteration, end_iteration,
            o[0].ctypes.data, c[0], C.addressof(ln[0]), trace.ctypes.data, len(trace), C.addressof(ntr)))
        return out, [int(x) for x in trace[:ntr.value]]

    # ---- the k-mer sorting stage (Count_<k>_sorted) on the same packed sets (rfx_dev_ksort_*)
    def ksort_params(self, k: int, **kw) -> "_lib.CKsortParams":
        """rfx_ksort_default_params (max_k 95, min_error_cov 8, max_cov 10000000, min_repeat_fold 1.5, bubble 1), then **kw"""
        return self._params(_lib.CKsortParams, self.L.rfx_ksort_default_params, "rfx_ksort_params", k, **kw)

    def ksort_binarize(self, d_text, d_row_off, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_ksort_binarize: `KMER,count` rows (torch uint8 tensor in HBM + int64 row offsets, n_rows + 1) -> two records per
        kept row"""
        n_rows = int(d_row_off.numel()) - 1
        return self._grow_call(self.L.rfx_dev_ksort_binarize, "rfx_dev_ksort_binarize", out or DynPacked(2 * n_rows, 2 * n_rows),
                                  lambda co: (d_text.data_ptr(), d_row_off.data_ptr(), n_rows, C.byref(params), C.byref(co)))

    def ksort_fork_filter(self, d: "DynPacked", reflected: bool, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_ksort_fork_filter over a sorted set: one survivor per run of equal keys"""
        ci = d._c()
        return self._grow_call(self.L.rfx_dev_ksort_fork_filter, "rfx_dev_ksort_fork_filter", out or DynPacked(d.n, d.n),
                                  lambda co: (int(reflected), C.byref(ci), C.byref(params), C.byref(co)))

    def ksort_reflect(self, d: "DynPacked", out: "DynPacked" = None) -> "DynPacked":
        ci = d._c()
        return self._grow_call(self.L.rfx_dev_ksort_reflect, "rfx_dev_ksort_reflect", out or DynPacked(d.n, d.n),
                                  lambda co: (C.byref(ci), C.byref(co)))

    def ksort_full_kmers(self, d: "DynPacked", out: "DynPacked" = None) -> "DynPacked":
        ci = d._c()
        return self._grow_call(self.L.rfx_dev_ksort_full_kmers, "rfx_dev_ksort_full_kmers", out or DynPacked(d.n, 0),
                                  lambda co: (C.byref(ci), C.byref(co)))

    def ksort_run(self, d_text, d_row_off, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_ksort_run: steps 1-8 with the set resident in HBM -> the full k-mers"""
        n_rows = int(d_row_off.numel()) - 1
        return self._grow_call(self.L.rfx_dev_ksort_run, "rfx_dev_ksort_run", out or DynPacked(2 * n_rows, 0),
                                  lambda co: (d_text.data_ptr(), d_row_off.data_ptr(), n_rows, C.byref(params), C.byref(co)))

    def _ksort_counts_call(self, fn, name, d_keys, d_counts, n, d_extra, n_extra, params, out):
        """the two entry points on the counter's arrays: keys (torch int64 in HBM, k // 32 + 1 words a row), counts (torch int32 or
        int64; its dtype is the count_bytes), extra keys of count 1 (None: none)"""
        n = int(d_counts.numel()) if n is None else int(n)
        W = int(params.k) // 32 + 1
        n_extra = (int(d_extra.numel()) // W if d_extra is not None else 0) if n_extra is None else int(n_extra)
        count_bytes = int(d_counts.element_size()) if d_counts is not None else 4
        out = out or DynPacked(2 * (n + n_extra), 0 if name.endswith("run_counts") else 2 * (n + n_extra))
        return self._grow_call(fn, name, out, lambda co: (
            d_keys.data_ptr() if d_keys is not None else None, d_counts.data_ptr() if d_counts is not None else None, count_bytes, n,
            d_extra.data_ptr() if d_extra is not None else None, n_extra, C.byref(params), C.byref(co)))

    def ksort_from_counts(self, d_keys, d_counts, params, n=None, d_extra=None, n_extra=None, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_ksort_from_counts: the counter's keys and counts in HBM (count_reads_ragged[_w]_dev), then the mercy k-mers (count
        1) -> the set ksort_binarize gives for their `KMER,count` rows, without the text"""
        return self._ksort_counts_call(self.L.rfx_dev_ksort_from_counts, "rfx_dev_ksort_from_counts", d_keys, d_counts, n, d_extra, n_extra,
                                       params, out)

    def ksort_run_counts(self, d_keys, d_counts, params, n=None, d_extra=None, n_extra=None, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_ksort_run_counts: steps 1-8 on the counter's arrays -> the full k-mers, as ksort_run on their rows"""
        return self._ksort_counts_call(self.L.rfx_dev_ksort_run_counts, "rfx_dev_ksort_run_counts", d_keys, d_counts, n, d_extra, n_extra,
                                       params, out)

    def ksort_to_text_dev(self, d: "DynPacked", k: int, d_text=None, want_offsets=True):
        """rfx_dev_ksort_to_text -> (torch uint8 tensor in HBM holding the rows "KMER,1|l|r\n", its length, the row offsets
        (torch int64 in HBM, rows + 1 entries in use; None without want_offsets), the rows)"""
        import torch
        ci = d._c()
        nr = C.c_int64(0)
        if d_text is None:
            d_text = torch.empty(max(1, (k + 24) * d.n), dtype=torch.uint8, device=d.key.device)
        d_off = torch.empty(d.n + 1, dtype=torch.int64, device=d.key.device) if want_offsets else None
        d_text, n = self._dev_text_call("rfx_dev_ksort_to_text", d_text, lambda t, ln: self.L.rfx_dev_ksort_to_text(
            self.ctx, C.byref(ci), int(k), t.data_ptr(), int(t.numel()), C.addressof(ln), d_off.data_ptr() if want_offsets else None,
            C.addressof(nr)))
        return d_text, n, d_off, int(nr.value)

    def ksort_text(self, text: bytes, params) -> bytes:
        """rfx_ksort_text: the rows of a counts file (bytes, one `KMER,count` row per line) -> the rows of Count_<k>_sorted"""
        text = bytes(text)
        off, n_rows = self._row_offsets(text)
        cap = 2 * (len(text) + 24 * n_rows) + 64
        return self._host_text_call("rfx_ksort_text", [cap], lambda o, c, ln: self.L.rfx_ksort_text(
            self.ctx, text, off.ctypes.data, n_rows, C.byref(params), o[0].ctypes.data, c[0], C.addressof(ln[0])))[0]

    # ---- the k-mer reduction stage (Count_<k1>_reduced, Count_<k2>_sorted / _reduced) on the same packed sets (rfx_dev_reduce_*,
    # DESIGN.md section 18)
    def reduce_params(self, k1: int, k2: int, **kw) -> "_lib.CReduceParams":
        """rfx_reduce_default_params (max_k = max(95, k2)), then **kw"""
        return self._params(_lib.CReduceParams, self.L.rfx_reduce_default_params, "rfx_reduce_params", k1, k2, **kw)

    def reduce_union(self, d_text_short, d_off_short, d_text_long, d_off_long, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_reduce_union: two `KMER,m|l|r` texts (torch uint8 tensors in HBM + int64 row offsets, rows + 1) -> the full k-mer
        records of the longer text, then the shorter one's"""
        ns, nl = int(d_off_short.numel()) - 1, int(d_off_long.numel()) - 1
        return self._grow_call(self.L.rfx_dev_reduce_union, "rfx_dev_reduce_union", out or DynPacked(ns + nl, 0),
                                  lambda co: (d_text_short.data_ptr(), d_off_short.data_ptr(), ns, d_text_long.data_ptr(), d_off_long.data_ptr(), nl,
                                              C.byref(params), C.byref(co)))

    def reduce_left_prepare(self, d: "DynPacked", params, out: "DynPacked" = None) -> "DynPacked":
        ci = d._c()
        return self._grow_call(self.L.rfx_dev_reduce_left_prepare, "rfx_dev_reduce_left_prepare", out or DynPacked(d.n, d.n),
                                  lambda co: (C.byref(ci), C.byref(params), C.byref(co)))

    def reduce_right_prepare(self, d: "DynPacked", params, out: "DynPacked" = None) -> "DynPacked":
        ci = d._c()
        return self._grow_call(self.L.rfx_dev_reduce_right_prepare, "rfx_dev_reduce_right_prepare", out or DynPacked(d.n, d.n),
                                  lambda co: (C.byref(ci), C.byref(params), C.byref(co)))

    def reduce_adjust(self, d: "DynPacked", right: bool, d_part_start, params, out: "DynPacked" = None):
        """rfx_dev_reduce_adjust over a sorted set and its partition starts -> (DynPacked, out_part_start: torch int64 [P + 1] in HBM)"""
        import torch
        ci = d._c()
        P = int(d_part_start.numel()) - 1
        ops = torch.empty(max(P, 0) + 1, dtype=torch.int64, device=d.key.device)
        out = self._grow_call(self.L.rfx_dev_reduce_adjust, "rfx_dev_reduce_adjust", out or DynPacked(d.n, d.n),
                                 lambda co: (int(right), C.byref(ci), d_part_start.data_ptr(), P, C.byref(params), C.byref(co), ops.data_ptr()))
        return out, ops

    def reduce_full_kmers(self, d: "DynPacked", params, out: "DynPacked" = None) -> "DynPacked":
        ci = d._c()
        return self._grow_call(self.L.rfx_dev_reduce_full_kmers, "rfx_dev_reduce_full_kmers", out or DynPacked(d.n, 0),
                                  lambda co: (C.byref(ci), C.byref(params), C.byref(co)))

    def reduce_neutralize(self, d: "DynPacked", d_part_start, params, out: "DynPacked" = None):
        """rfx_dev_reduce_neutralize over a sorted set of full k-mers -> (DynPacked, out_part_start: torch int64 [P + 1] in HBM)"""
        import torch
        ci = d._c()
        P = int(d_part_start.numel()) - 1
        ops = torch.empty(max(P, 0) + 1, dtype=torch.int64, device=d.key.device)
        out = self._grow_call(self.L.rfx_dev_reduce_neutralize, "rfx_dev_reduce_neutralize", out or DynPacked(d.n, 0),
                                 lambda co: (C.byref(ci), d_part_start.data_ptr(), P, C.byref(params), C.byref(co), ops.data_ptr()))
        return out, ops

    def reduce_run(self, d_text_short, d_off_short, d_text_long, d_off_long, P: int, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_reduce_run: the whole driver with the set resident in HBM -> the final full k-mers (both lengths; the two
        output texts are ksort_to_text_dev of it with k = k1 and with k = k2)"""
        ns, nl = int(d_off_short.numel()) - 1, int(d_off_long.numel()) - 1
        return self._grow_call(self.L.rfx_dev_reduce_run, "rfx_dev_reduce_run", out or DynPacked(ns + nl, 0),
                                  lambda co: (d_text_short.data_ptr(), d_off_short.data_ptr(), ns, d_text_long.data_ptr(), d_off_long.data_ptr(), nl,
                                              int(P), C.byref(params), C.byref(co)))

    def reduce_union_packed(self, short: "DynPacked", long: "DynPacked", params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_reduce_union_packed: two packed sets of full k-mers (ksort_run / reduce_run results) -> what reduce_union gives for
        their ksort_to_text_dev texts (k1 of `short`, k2 of `long`), without the texts"""
        cs, cl = short._c(), long._c()
        return self._grow_call(self.L.rfx_dev_reduce_union_packed, "rfx_dev_reduce_union_packed", out or DynPacked(short.n + long.n, 0),
                                  lambda co: (C.byref(cs), C.byref(cl), C.byref(params), C.byref(co)))

    def reduce_run_packed(self, short: "DynPacked", long: "DynPacked", P: int, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_reduce_run_packed: the whole driver on two packed sets of full k-mers -> the final full k-mers (both lengths)"""
        cs, cl = short._c(), long._c()
        return self._grow_call(self.L.rfx_dev_reduce_run_packed, "rfx_dev_reduce_run_packed", out or DynPacked(short.n + long.n, 0),
                                  lambda co: (C.byref(cs), C.byref(cl), int(P), C.byref(params), C.byref(co)))

    def dyn_from_kmers(self, sets, key_lens, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_dyn_from_kmers: packed sets of full k-mers and one key length each -> set after set, the sub-k-mer records
        dyn_binarize_dev form 0 gives for the ksort_to_text_dev rows of that length"""
        sets, key_lens = list(sets), [int(x) for x in key_lens]
        assert len(sets) == len(key_lens)
        m = len(sets)
        arr = (_lib.CDynPacked * max(m, 1))(*[s._c() for s in sets])
        lens = (C.c_int * max(m, 1))(*key_lens)
        total = sum(s.n for s in sets)
        return self._grow_call(self.L.rfx_dev_dyn_from_kmers, "rfx_dev_dyn_from_kmers", out or DynPacked(total, total),
                                  lambda co: (C.addressof(arr), C.addressof(lens), m, C.byref(co)))

    def reduce_reads_params(self, **kw) -> "_lib.CReduceReadsParams":
        """rfx_reduce_reads_default_params (min_cov 2, max_cov 10000000, min_error_cov 8, min_repeat_fold 1.5, bubble 1, sensitive 0,
        no clips, P 8), then **kw"""
        return self._params(_lib.CReduceReadsParams, self.L.rfx_reduce_reads_default_params, "rfx_reduce_reads_params", **kw)

    def reduce_reads_dev(self, d_words, d_read_len, n_reads: int, words_per_read: int, max_read_len: int, klist, params=None,
                         out: "DynPacked" = None):
        """rfx_dev_reduce_reads: the 2-bit read store in HBM (torch tensors, as encode_reads_dev writes them) and a k list -> (the set of
        the first-four passes: the sub-k-mer records of every Count_<k>_reduced in list order, [each k's row count]).  A set that
        turns out too small is regrown and the call made again."""
        klist = [int(k) for k in klist]
        params = params or self.reduce_reads_params()
        ks = (C.c_int * max(len(klist), 1))(*klist)
        per_k = (C.c_int64 * max(len(klist), 1))()
        out = self._grow_call(self.L.rfx_dev_reduce_reads, "rfx_dev_reduce_reads", out or DynPacked(1 << 16, 1 << 16), lambda co: (
            d_words.data_ptr() if d_words is not None else None, d_read_len.data_ptr() if d_read_len is not None else None, int(n_reads),
            int(words_per_read), int(max_read_len), C.addressof(ks), len(klist), C.byref(params), C.byref(co), C.addressof(per_k)))
        return out, [int(x) for x in per_k[:len(klist)]]

    def reduce_reads_text(self, reads, klist, params=None):
        """rfx_reduce_reads: the reads -- a list of bytes, or (the bases as one numpy uint8 array, the n + 1 int64 offsets) -- and a k
        list -> [the rows of Count_<k>_reduced as bytes, one entry per k]; one upload, everything between in HBM"""
        klist = [int(k) for k in klist]
        params = params or self.reduce_reads_params()
        if isinstance(reads, tuple):
            bases, off = np.ascontiguousarray(reads[0], np.uint8), np.ascontiguousarray(reads[1], np.int64)
        else:
            reads = [bytes(r) for r in reads]
            bases = np.frombuffer(b"".join(reads), np.uint8) if reads else np.zeros(0, np.uint8)
            off = np.zeros(len(reads) + 1, np.int64)
            off[1:] = np.cumsum([len(r) for r in reads])
        n = len(off) - 1
        bases = bases if len(bases) else np.zeros(1, np.uint8)
        ks = (C.c_int * max(len(klist), 1))(*klist)
        offs = np.zeros(len(klist) + 1, np.int64)
        text, = self._host_text_call("rfx_reduce_reads", [max(1 << 16, 4 * len(bases))], lambda o, c, ln: self.L.rfx_reduce_reads(
            self.ctx, bases.ctypes.data, off.ctypes.data, n, C.addressof(ks), len(klist), C.byref(params), o[0].ctypes.data, c[0], C.addressof(ln[0]),
            offs.ctypes.data))
        return [text[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]

    # ---- reads to contigs in one resident call (rfx_dev_meta_*, rfx_meta_reads)
    def meta_params(self, **kw) -> "_lib.CMetaParams":
        """rfx_meta_default_params (P 8, scramble 2, max_iteration 150, min_contig 500, the mapper's 21 / 31 / 2, stop_after Assembly),
        then **kw; stop_after may be a name of _lib.META_STAGES"""
        if isinstance(kw.get("stop_after"), str):
            kw["stop_after"] = _lib.META_STAGES.index(kw["stop_after"])
        return self._params(_lib.CMetaParams, self.L.rfx_meta_default_params, "rfx_meta_params", **kw)

    @staticmethod
    def _meta_report(rep) -> dict:
        out = {name: int(rep.n[i]) for i, name in enumerate(_lib.META_STAGES)}
        out["reduced"], out["hits"] = int(rep.n_reduced), int(rep.hits)
        return out

    def meta_from_reduced_dev(self, reduced: "DynPacked", d_words, d_read_len, n_reads: int, words_per_read: int, max_k: int, params=None,
                              out: "ContigsPacked" = None):
        """rfx_dev_meta_from_reduced: the set reduce_reads_dev leaves and the read store -> (the de-duplicated contigs as a ContigsPacked,
        the report as a dict: stage name -> records or contigs left, "reduced", "hits").  A set that turns out too small is regrown and
        the call made again."""
        params = params or self.meta_params()
        ci, rep = reduced._c(), _lib.CMetaReport()
        out = self._grow_call(self.L.rfx_dev_meta_from_reduced, "rfx_dev_meta_from_reduced", out or ContigsPacked(1 << 12, 1 << 16, reduced.key.device), lambda co: (
            C.byref(ci), d_words.data_ptr() if d_words is not None else None, d_read_len.data_ptr() if d_read_len is not None else None, int(n_reads),
            int(words_per_read), int(max_k), C.byref(params), C.byref(rep), C.byref(co)), reduced.key.device)
        return out, self._meta_report(rep)

    def meta_reads_dev(self, d_words, d_read_len, n_reads: int, words_per_read: int, max_read_len: int, klist, reduce_params=None, params=None,
                       out: "ContigsPacked" = None):
        """rfx_dev_meta_reads: the 2-bit read store in HBM and a k list -> (the de-duplicated contigs, the report)"""
        klist = [int(k) for k in klist]
        reduce_params, params = reduce_params or self.reduce_reads_params(), params or self.meta_params()
        ks = (C.c_int * max(len(klist), 1))(*klist)
        rep = _lib.CMetaReport()
        out = self._grow_call(self.L.rfx_dev_meta_reads, "rfx_dev_meta_reads", out or ContigsPacked(1 << 12, 1 << 16), lambda co: (
            d_words.data_ptr() if d_words is not None else None, d_read_len.data_ptr() if d_read_len is not None else None, int(n_reads),
            int(words_per_read), int(max_read_len), C.addressof(ks), len(klist), C.byref(reduce_params), C.byref(params), C.byref(rep), C.byref(co)))
        return out, self._meta_report(rep)

    def meta_reads_text(self, reads, klist, reduce_params=None, params=None, with_report=False):
        """rfx_meta_reads: the reads -- a list of bytes, or (the bases as one numpy uint8 array, the n + 1 int64 offsets) -- and a k list ->
        the file of the stage params.stop_after names, as bytes (and the report); one upload, everything between in HBM"""
        klist = [int(k) for k in klist]
        reduce_params, params = reduce_params or self.reduce_reads_params(), params or self.meta_params()
        if isinstance(reads, tuple):
            bases, off = np.ascontiguousarray(reads[0], np.uint8), np.ascontiguousarray(reads[1], np.int64)
        else:
            reads = [bytes(r) for r in reads]
            bases = np.frombuffer(b"".join(reads), np.uint8) if reads else np.zeros(0, np.uint8)
            off = np.zeros(len(reads) + 1, np.int64)
            off[1:] = np.cumsum([len(r) for r in reads])
        n = len(off) - 1
        bases = bases if len(bases) else np.zeros(1, np.uint8)
        ks = (C.c_int * max(len(klist), 1))(*klist)
        rep = _lib.CMetaReport()
        text, = self._host_text_call("rfx_meta_reads", [max(1 << 16, 2 * len(bases))], lambda o, c, ln: self.L.rfx_meta_reads(
            self.ctx, bases.ctypes.data, off.ctypes.data, n, C.addressof(ks), len(klist), C.byref(reduce_params), C.byref(params), C.byref(rep),
            o[0].ctypes.data, c[0], C.addressof(ln[0])))
        return (text, self._meta_report(rep)) if with_report else text

    @staticmethod
    def _row_offsets(text: bytes):
        buf = np.frombuffer(text, np.uint8)
        ends = np.flatnonzero(buf == 10)
        starts = np.concatenate([[0], ends + 1]).astype(np.int64)
        starts = starts[starts < len(buf)]
        return np.concatenate([starts, [len(buf)]]).astype(np.int64), len(starts)

    def reduce_text(self, text_short: bytes, text_long: bytes, P: int, params):
        """rfx_reduce_text: the rows of Count_<k1>_sorted and Count_<k2>_sorted (bytes, one `KMER,m|l|r` row per line) -> (the rows
        of Count_<k1>_reduced, the rows of the rewritten Count_<k2>_sorted / Count_<k2>_reduced)"""
        ts, tl = bytes(text_short), bytes(text_long)
        offs, ns = self._row_offsets(ts)
        offl, nl = self._row_offsets(tl)
        cap1, cap2 = len(ts) + ns + 64, len(tl) + nl + 64      # (an edited marker may grow a row by one character)
        return tuple(self._host_text_call("rfx_reduce_text", [cap1, cap2], lambda o, c, ln: self.L.rfx_reduce_text(
            self.ctx, ts, offs.ctypes.data, ns, tl, offl.ctypes.data, nl, int(P), C.byref(params), o[0].ctypes.data, c[0], C.addressof(ln[0]),
            o[1].ctypes.data, c[1], C.addressof(ln[1]))))

    # ---- the contig fixing stage (Assembly_intermediate/04Fixing) on the same packed sets (rfx_dev_fix_*)
    def fix_params(self, max_k: int, **kw) -> "_lib.CFixParams":
        """rfx_fix_default_params (scramble 2, max_iteration 150), then **kw"""
        return self._params(_lib.CFixParams, self.L.rfx_fix_default_params, "rfx_fix_params", max_k, **kw)

    def fix_binarize(self, d_text, d_row_off, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_fix_binarize: `SUBKMER,m|l|r,EXTENSION` rows (torch uint8 tensor in HBM + int64 row offsets, n_rows + 1) -> the
        records of the rows that hold 2 max_k bases or more"""
        n_rows = int(d_row_off.numel()) - 1
        return self._grow_call(self.L.rfx_dev_fix_binarize, "rfx_dev_fix_binarize", out or DynPacked(n_rows, n_rows + int(d_text.numel()) // 32),
                                  lambda co: (d_text.data_ptr(), d_row_off.data_ptr(), n_rows, C.byref(params), C.byref(co)))

    def fix_contig_ends(self, d: "DynPacked", params, out: "DynPacked" = None, d_kmers=None):
        """rfx_dev_fix_contig_ends -> (the long records: the trimmed contigs cut key 30 / rest, the end 31-mers in emission order:
        torch int64 tensor in HBM holding 62-bit values, their count)"""
        import torch
        ci = d._c()
        if d_kmers is None:
            d_kmers = torch.empty(max(1, 2 * (int(params.max_k) - 30) * d.n), dtype=torch.int64, device=d.key.device)
        return self._contig_ends_call(self.L.rfx_dev_fix_contig_ends, "rfx_dev_fix_contig_ends", ci, params, out or DynPacked(d.n, d.words + 4 * d.n),
                                      d_kmers, None, d.key.device)

    def _contig_ends_call(self, fn, name, ci, params, out: "DynPacked", d_kmers, device, kmers_device):
        """the call of fix_contig_ends / ext_contig_ends: the long records into `out` and the end 31-mers into d_kmers, each regrown on
        its own when the call reports that it is short -> (out, d_kmers, the 31-mers' count)"""
        import torch
        nk = C.c_int64(0)
        km = [d_kmers]

        def regrow_kmers():
            if nk.value > km[0].numel():
                km[0] = torch.empty(nk.value, dtype=torch.int64, device=kmers_device)
        out = self._grow_call(fn, name, out, lambda co: (C.byref(ci), C.byref(params), C.byref(co), km[0].data_ptr(), int(km[0].numel()), C.addressof(nk)),
                              device, regrow_kmers)
        return out, km[0], int(nk.value)

    def fix_kmer_set(self, d_kmers, n_kmers: int, d_long: "DynPacked", out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_fix_kmer_set: the distinct 31-mers as one-base records (ascending), then the long records"""
        ci = d_long._c()
        out = out or DynPacked(n_kmers + d_long.n, n_kmers + d_long.words)
        return self._grow_call(self.L.rfx_dev_fix_kmer_set, "rfx_dev_fix_kmer_set", out,
                                  lambda co: (d_kmers.data_ptr() if n_kmers else None, int(n_kmers), C.byref(ci), C.byref(co)))

    def fix_fork_filter(self, d: "DynPacked", reflected: bool, d_part_start, out: "DynPacked" = None):
        """rfx_dev_fix_fork_filter over a sorted set and its partition starts -> (DynPacked, out_part_start: torch int64 [P + 1] in HBM)"""
        import torch
        ci = d._c()
        P = int(d_part_start.numel()) - 1
        ops = torch.empty(max(P, 0) + 1, dtype=torch.int64, device=d.key.device)
        out = self._grow_call(self.L.rfx_dev_fix_fork_filter, "rfx_dev_fix_fork_filter", out or DynPacked(d.n, d.words),
                                 lambda co: (int(reflected), C.byref(ci), d_part_start.data_ptr(), P, C.byref(co), ops.data_ptr()))
        return out, ops

    def fix_reflect(self, d: "DynPacked", out: "DynPacked" = None) -> "DynPacked":
        ci = d._c()
        return self._grow_call(self.L.rfx_dev_fix_reflect, "rfx_dev_fix_reflect", out or DynPacked(d.n, d.words),
                                  lambda co: (C.byref(ci), C.byref(co)))

    def fix_run(self, d_text, d_row_off, P: int, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_fix_run: steps 1-9 with the set resident in HBM -> the set behind the last loop pass (the output file is
        dyn_to_text_dev of it)"""
        n_rows = int(d_row_off.numel()) - 1
        cap_n = n_rows * (2 * (int(params.max_k) - 30) + 1)
        return self._grow_call(self.L.rfx_dev_fix_run, "rfx_dev_fix_run", out or DynPacked(cap_n, cap_n + int(d_text.numel()) // 32),
                                  lambda co: (d_text.data_ptr(), d_row_off.data_ptr(), n_rows, int(P), C.byref(params), C.byref(co)))

    def fix_run_packed(self, d: "DynPacked", P: int, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_fix_run_packed: fix_run on the rows dyn_to_text_dev would write of `d`, with no text made -- the last iteration's
        set feeds it as it is"""
        ci = d._c()
        cap_n = d.n * (2 * (int(params.max_k) - 30) + 1)
        return self._grow_call(self.L.rfx_dev_fix_run_packed, "rfx_dev_fix_run_packed", out or DynPacked(cap_n, cap_n + d.words + 4 * d.n),
                                  lambda co: (C.byref(ci), int(P), C.byref(params), C.byref(co)))

    def fix_text(self, text: bytes, P: int, params) -> bytes:
        """rfx_fix_text: the rows of the last iteration's output (bytes, one `SUBKMER,m|l|r,EXTENSION` row per line) -> the rows of
        04Fixing"""
        text = bytes(text)
        off, n_rows = self._row_offsets(text)
        cap = len(text) + 48 * n_rows * (2 * (int(params.max_k) - 30) + 1) + 64
        return self._host_text_call("rfx_fix_text", [cap], lambda o, c, ln: self.L.rfx_fix_text(
            self.ctx, text, off.ctypes.data, n_rows, int(P), C.byref(params), o[0].ctypes.data, c[0], C.addressof(ln[0])))[0]

    # ---- the second contig fixing stage (05FixingAgain, 06ContigEnds) on the same packed sets (rfx_dev_fix2_*)
    def fix2_binarize(self, d_text, d_row_off, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_fix2_binarize: the rows of 04Fixing (torch uint8 tensor in HBM + int64 row offsets, n_rows + 1) -> their records;
        no length filter"""
        n_rows = int(d_row_off.numel()) - 1
        return self._grow_call(self.L.rfx_dev_fix2_binarize, "rfx_dev_fix2_binarize", out or DynPacked(n_rows, n_rows + int(d_text.numel()) // 32),
                                  lambda co: (d_text.data_ptr(), d_row_off.data_ptr(), n_rows, C.byref(co)))

    def fix2_run(self, d: "DynPacked", P: int, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_fix2_run: min(max_iteration + 1, 29) x (sort, loop) on a packed set -- the output of fix_run feeds it as it is"""
        ci = d._c()
        return self._grow_call(self.L.rfx_dev_fix2_run, "rfx_dev_fix2_run", out or DynPacked(d.n, d.words),
                                  lambda co: (C.byref(ci), int(P), C.byref(params), C.byref(co)))

    def fix2_contigs(self, d: "DynPacked", params, out: "ContigsPacked" = None, d_left=None, d_right=None):
        """rfx_dev_fix2_contigs -> (the contigs of at least 2 max_k bases as a ContigsPacked, left, right: torch int32 tensors in HBM,
        cap_n entries each)"""
        import torch
        ci = d._c()
        lr = [d_left, d_right]

        def args(co):                      # left / right follow the capacity of the set each attempt writes
            for i in (0, 1):
                if lr[i] is None or lr[i].numel() < max(1, int(co.cap_n)):
                    lr[i] = torch.empty(max(1, int(co.cap_n)), dtype=torch.int32, device=d.key.device)
            return (C.byref(ci), C.byref(params), C.byref(co), lr[0].data_ptr(), lr[1].data_ptr())
        out = self._grow_call(self.L.rfx_dev_fix2_contigs, "rfx_dev_fix2_contigs", out or ContigsPacked(d.n, d.words + 4 * d.n, d.key.device), args,
                              d.key.device)
        return out, lr[0], lr[1]

    def _fix2_text_dev(self, fn, name, c: "ContigsPacked", d_left, d_right, d_text):
        import torch
        ci = c._c()
        if d_text is None:
            d_text = torch.empty(max(1, 96 * c.n + 32 * c.words + 64), dtype=torch.uint8, device=c.word_off.device)
        return self._dev_text_call(name, d_text, lambda t, ln: fn(
            self.ctx, C.byref(ci), d_left.data_ptr(), d_right.data_ptr(), t.data_ptr(), int(t.numel()), C.addressof(ln)))

    def fix2_to_text(self, c: "ContigsPacked", d_left, d_right, d_text=None):
        """rfx_dev_fix2_to_text -> (torch uint8 tensor in HBM holding the rows "Contig_<L>_<left>_<right>_<idx>,<contig>\\n" of
        05FixingAgain, its length)"""
        return self._fix2_text_dev(self.L.rfx_dev_fix2_to_text, "rfx_dev_fix2_to_text", c, d_left, d_right, d_text)

    def fix2_ends_text(self, c: "ContigsPacked", d_left, d_right, d_text=None):
        """rfx_dev_fix2_ends_text -> (torch uint8 tensor in HBM holding the lines of 06ContigEnds, its length)"""
        return self._fix2_text_dev(self.L.rfx_dev_fix2_ends_text, "rfx_dev_fix2_ends_text", c, d_left, d_right, d_text)

    def fix2_text(self, text: bytes, P: int, params):
        """rfx_fix2_text: the rows of 04Fixing (bytes, one `SUBKMER,m|l|r,EXTENSION` row per line) -> (the rows of 05FixingAgain, the
        lines of 06ContigEnds), both as bytes"""
        text = bytes(text)
        off, n_rows = self._row_offsets(text)
        cap1 = cap2 = len(text) + 64 * n_rows + 64
        return tuple(self._host_text_call("rfx_fix2_text", [cap1, cap2], lambda o, c, ln: self.L.rfx_fix2_text(
            self.ctx, text, off.ctypes.data, n_rows, int(P), C.byref(params), o[0].ctypes.data, c[0], C.addressof(ln[0]), o[1].ctypes.data, c[1],
            C.addressof(ln[1]))))

    # ---- the end extension of contigs from alignment rows (07EndExtend) on packed sets (rfx_dev_endext_*)
    def endext_consensus(self, c: "ContigsPacked", d_left, d_right, d_text, d_row_off, out: "EndextConsensus" = None) -> "EndextConsensus":
        """rfx_dev_endext_consensus: the contigs rfx_dev_fix2_contigs returns + alignment rows "name \\t start \\t cigar \\t seq" (torch
        uint8 tensor in HBM + int64 row offsets, n_rows + 1) -> the consensus of both ends of every contig, and its flags"""
        ci = c._c()
        n_rows = int(d_row_off.numel()) - 1
        return self._grow_call(self.L.rfx_dev_endext_consensus, "rfx_dev_endext_consensus", out or EndextConsensus(c.n, device=c.word_off.device),
                               lambda co: (C.byref(ci), d_left.data_ptr(), d_right.data_ptr(), d_text.data_ptr(), d_row_off.data_ptr(), n_rows, C.byref(co)),
                               c.word_off.device)

    def endext_consensus_hits(self, c: "ContigsPacked", d_left, d_right, d_words, d_read_len, words_per_read: int, hits: "MapHits",
                              out: "EndextConsensus" = None) -> "EndextConsensus":
        """rfx_dev_endext_consensus_hits: endext_consensus on the rows map_to_text would write for these contigs, reads and hits, with no
        text made"""
        ci, ch = c._c(), hits._c()
        return self._grow_call(self.L.rfx_dev_endext_consensus_hits, "rfx_dev_endext_consensus_hits", out or EndextConsensus(c.n, device=c.word_off.device),
                               lambda co: (C.byref(ci), d_left.data_ptr(), d_right.data_ptr(), d_words.data_ptr(), d_read_len.data_ptr(), int(words_per_read),
                                           C.byref(ch), C.byref(co)), c.word_off.device)

    def endext_contigs(self, c: "ContigsPacked", d_left, d_right, cons: "EndextConsensus", max_k: int, out: "EndextSet" = None) -> "EndextSet":
        """rfx_dev_endext_contigs: the splice and the order -> the contigs of 07EndExtend, in output order, with their arrays"""
        ci, cc = c._c(), cons._c()
        return self._grow_call(self.L.rfx_dev_endext_contigs, "rfx_dev_endext_contigs", out or EndextSet(c.n, c.words + 21 * c.n, c.word_off.device),
                               lambda co: (C.byref(ci), d_left.data_ptr(), d_right.data_ptr(), C.byref(cc), int(max_k), C.byref(co)), c.word_off.device)

    def endext_to_text(self, s: "EndextSet", d_text=None):
        """rfx_dev_endext_to_text -> (torch uint8 tensor in HBM holding the rows of 07EndExtend, its length)"""
        import torch
        ci = s._c()
        if d_text is None:
            d_text = torch.empty(max(1, 128 * s.n + 32 * s.set.words + 64), dtype=torch.uint8, device=s.set.word_off.device)
        return self._dev_text_call("rfx_dev_endext_to_text", d_text, lambda t, ln: self.L.rfx_dev_endext_to_text(
            self.ctx, C.byref(ci), t.data_ptr(), int(t.numel()), C.addressof(ln)))

    def endext_text(self, contig_text: bytes, row_text: bytes, max_k: int) -> bytes:
        """rfx_endext_text: the rows of 05FixingAgain and the alignment rows (bytes, one row per line) -> the rows of 07EndExtend"""
        ct, rt = bytes(contig_text), bytes(row_text)
        offc, nc = self._row_offsets(ct)
        offr, nr = self._row_offsets(rt)
        cap = len(ct) + 700 * nc + 64
        return self._host_text_call("rfx_endext_text", [cap], lambda o, c, ln: self.L.rfx_endext_text(
            self.ctx, ct, offc.ctypes.data, nc, rt, offr.ctypes.data, nr, int(max_k), o[0].ctypes.data, c[0], C.addressof(ln[0])))[0]

    # ---- reads onto the contig ends, the front half of the Mapping stage (rfx_dev_map_*)
    def map_params(self, **kw) -> "_lib.CMapParams":
        """rfx_map_default_params (seed 21, min_overlap 31, max_mismatch 2), then **kw"""
        return self._params(_lib.CMapParams, self.L.rfx_map_default_params, "rfx_map_params", **kw)

    def map_ends(self, c: "ContigsPacked", d_left, d_right, d_words, d_read_len, n_reads: int, words_per_read: int, params=None,
                 out: "MapHits" = None) -> "MapHits":
        """rfx_dev_map_ends: the contigs rfx_dev_fix2_contigs returns + the 2-bit read store (torch tensors in HBM: the words as int64 bit
        patterns, the lengths as int32 bit patterns of uint32) -> the rows that hang over a contig end, in row order"""
        ci = c._c()
        params = params or self.map_params()
        out = out or MapHits(64 + int(n_reads) // 2, c.word_off.device)     # (a short one is replaced by one of the need the call reports)
        return self._grow_call(self.L.rfx_dev_map_ends, "rfx_dev_map_ends", out, lambda co: (
            C.byref(ci), d_left.data_ptr(), d_right.data_ptr(), d_words.data_ptr(), d_read_len.data_ptr(), int(n_reads), int(words_per_read),
            C.byref(params), C.byref(co)), c.word_off.device)

    def map_to_text(self, c: "ContigsPacked", d_left, d_right, d_words, d_read_len, words_per_read: int, hits: "MapHits", d_text=None):
        """rfx_dev_map_to_text -> (torch uint8 tensor in HBM holding the rows "name \\t start \\t cigar \\t seq \\n", its length, the
        int64 row offsets, hits.n + 1) -- what endext_consensus takes"""
        import torch
        ci, ch = c._c(), hits._c()
        dev = c.word_off.device
        d_row_off = torch.empty(hits.n + 1, dtype=torch.int64, device=dev)
        if d_text is None:
            d_text = torch.empty(max(1, hits.n * (32 * int(words_per_read) + 96)), dtype=torch.uint8, device=dev)
        d_text, ln = self._dev_text_call("rfx_dev_map_to_text", d_text, lambda t, ln: self.L.rfx_dev_map_to_text(
            self.ctx, C.byref(ci), d_left.data_ptr(), d_right.data_ptr(), d_words.data_ptr(), d_read_len.data_ptr(), int(words_per_read), C.byref(ch),
            t.data_ptr(), int(t.numel()), C.addressof(ln), d_row_off.data_ptr(), int(d_row_off.numel())))
        return d_text, ln, d_row_off

    def map_text(self, contig_text: bytes, reads, params=None) -> bytes:
        """rfx_map_text: the rows of 05FixingAgain (bytes, one row per line) and the reads -- a list of bytes, or (the bases as one
        numpy uint8 array, the n + 1 int64 offsets) -- -> the row text"""
        ct = bytes(contig_text)
        offc, nc = self._row_offsets(ct)
        params = params or self.map_params()
        if isinstance(reads, tuple):
            bases, offr = np.ascontiguousarray(reads[0], np.uint8), np.ascontiguousarray(reads[1], np.int64)
        else:
            reads = [bytes(r) for r in reads]
            bases = np.frombuffer(b"".join(reads), np.uint8)
            offr = np.zeros(len(reads) + 1, np.int64)
            np.cumsum([len(r) for r in reads], out=offr[1:])
        nr = len(offr) - 1
        cap = 4 * len(bases) + 256 * nr + 64
        return self._host_text_call("rfx_map_text", [cap], lambda o, c, ln: self.L.rfx_map_text(
            self.ctx, ct, offc.ctypes.data, nc, bases.ctypes.data, offr.ctypes.data, nr, C.byref(params), o[0].ctypes.data, c[0],
            C.addressof(ln[0])))[0]

    # ---- the mercy k-mer stage (Count_<k>_mercy) on the read store (rfx_dev_mercy_*)
    def mercy_kmers(self, d_solid_keys, n_solid: int, d_words, d_read_len, n_reads: int, words_per_read: int, k: int, front_clip=0, end_clip=0,
                    out: "MercyKmers" = None) -> "MercyKmers":
        """rfx_dev_mercy_kmers: the counter's surviving keys (ascending) + the 2-bit read store (torch tensors in HBM: keys and words as
        int64 bit patterns, the lengths as int32 bit patterns of uint32) -> the k-mers of the holes between two solid windows of a read"""
        out = out or MercyKmers(64 + int(n_reads), d_words.device)      # (a short one is replaced by one of the need the call reports)
        return self._grow_call(self.L.rfx_dev_mercy_kmers, "rfx_dev_mercy_kmers", out, lambda co: (
            d_solid_keys.data_ptr(), int(n_solid), d_words.data_ptr(), d_read_len.data_ptr(), int(n_reads), int(words_per_read), int(k),
            int(front_clip), int(end_clip), co.keys, co.cap_n, C.addressof(co.n)), d_words.device)

    def mercy_to_text(self, keys, n: int, k: int, d_text=None, want_offsets=True):
        """rfx_dev_mercy_to_text: n keys (a MercyKmers' tensor, or any torch int64 tensor in HBM) -> (torch uint8 tensor in HBM holding
        the rows "KMER,1\\n", its length, the n + 1 int64 row offsets in HBM or None) -- what ksort_binarize takes"""
        import torch
        n = int(n)
        d_off = torch.empty(n + 1, dtype=torch.int64, device=keys.device) if want_offsets else None
        if d_text is None:
            d_text = torch.empty(max(1, n * (int(k) + 3)), dtype=torch.uint8, device=keys.device)
        d_text, ln = self._dev_text_call("rfx_dev_mercy_to_text", d_text, lambda t, ln: self.L.rfx_dev_mercy_to_text(
            self.ctx, keys.data_ptr(), n, int(k), t.data_ptr(), int(t.numel()), C.addressof(ln), d_off.data_ptr() if want_offsets else None))
        return d_text, ln, d_off

    def mercy_text(self, count_text: bytes, reads, k: int, front_clip=0, end_clip=0) -> bytes:
        """rfx_mercy_text: the rows of Count_<k> (bytes, one `KMER,count` row per line, in any order) and the reads -- a list of bytes, or
        (the bases as one numpy uint8 array, the n + 1 int64 offsets) -- -> the rows of Count_<k>_mercy"""
        ct = bytes(count_text)
        offc, nc = self._row_offsets(ct)
        if isinstance(reads, tuple):
            bases, offr = np.ascontiguousarray(reads[0], np.uint8), np.ascontiguousarray(reads[1], np.int64)
        else:
            reads = [bytes(r) for r in reads]
            bases = np.frombuffer(b"".join(reads), np.uint8)
            offr = np.zeros(len(reads) + 1, np.int64)
            np.cumsum([len(r) for r in reads], out=offr[1:])
        nr = len(offr) - 1
        cap = (int(k) + 3) * (nr + 64)
        return self._host_text_call("rfx_mercy_text", [cap], lambda o, c, ln: self.L.rfx_mercy_text(
            self.ctx, ct, offc.ctypes.data, nc, bases.ctypes.data, offr.ctypes.data, nr, int(k), int(front_clip), int(end_clip),
            o[0].ctypes.data, c[0], C.addressof(ln[0])))[0]

    # ---- the contig extension stages (08Extend, 09ExtendAgain) on packed sets (rfx_dev_ext_*, rfx_dev_ext2_*)
    def ext_from_text(self, d_text, d_row_off, params, out: "EndextSet" = None) -> "EndextSet":
        """rfx_dev_ext_from_text: the rows of 07EndExtend (torch uint8 tensor in HBM + int64 row offsets, n_rows + 1) -> the set of the
        rows of at least 2 max_k characters, the literals of a flagged seam as T bases, flags 0"""
        n_rows = int(d_row_off.numel()) - 1
        return self._grow_call(self.L.rfx_dev_ext_from_text, "rfx_dev_ext_from_text", out or EndextSet(n_rows, n_rows + int(d_text.numel()) // 32, d_text.device),
                               lambda co: (d_text.data_ptr(), d_row_off.data_ptr(), n_rows, C.byref(params), C.byref(co)), d_text.device)

    def ext_contig_ends(self, s: "EndextSet", params, out: "DynPacked" = None, d_kmers=None):
        """rfx_dev_ext_contig_ends -> (the long records: the cut contigs, key 30 / rest, the end 31-mers in emission order: torch int64
        tensor in HBM holding 62-bit values, their count)"""
        import torch
        ci = s._c()
        dev = s.set.word_off.device
        if d_kmers is None:
            d_kmers = torch.empty(max(1, 606 * s.n), dtype=torch.int64, device=dev)
        return self._contig_ends_call(self.L.rfx_dev_ext_contig_ends, "rfx_dev_ext_contig_ends", ci, params, out or DynPacked(s.n, s.set.words, dev),
                                      d_kmers, dev, dev)

    def ext_run(self, s: "EndextSet", P: int, params, out: "DynPacked" = None) -> "DynPacked":
        """rfx_dev_ext_run: 08Extend with the set resident in HBM -> the set behind the last loop pass (the output file is
        dyn_to_text_dev of it; fix2_run takes it as it is)"""
        ci = s._c()
        cap_n = 607 * s.n
        return self._grow_call(self.L.rfx_dev_ext_run, "rfx_dev_ext_run", out or DynPacked(cap_n, cap_n + s.set.words, s.set.word_off.device),
                                  lambda co: (C.byref(ci), int(P), C.byref(params), C.byref(co)))

    def ext_text(self, text: bytes, P: int, params) -> bytes:
        """rfx_ext_text: the rows of 07EndExtend (bytes, one row per line) -> the rows of 08Extend"""
        text = bytes(text)
        off, n_rows = self._row_offsets(text)
        cap = len(text) + 48 * 607 * n_rows + 64
        return self._host_text_call("rfx_ext_text", [cap], lambda o, c, ln: self.L.rfx_ext_text(
            self.ctx, text, off.ctypes.data, n_rows, int(P), C.byref(params), o[0].ctypes.data, c[0], C.addressof(ln[0])))[0]

    def ext2_to_text(self, c: "ContigsPacked", d_text=None):
        """rfx_dev_ext2_to_text -> (torch uint8 tensor in HBM holding the rows ">Contig-<len>-<idx>,<contig>\n" of 09ExtendAgain, its
        length)"""
        import torch
        ci = c._c()
        if d_text is None:
            d_text = torch.empty(max(1, 48 * c.n + 32 * c.words + 64), dtype=torch.uint8, device=c.word_off.device)
        return self._dev_text_call("rfx_dev_ext2_to_text", d_text, lambda t, ln: self.L.rfx_dev_ext2_to_text(
            self.ctx, C.byref(ci), t.data_ptr(), int(t.numel()), C.addressof(ln)))

    def ext2_text(self, text: bytes, P: int, params) -> bytes:
        """rfx_ext2_text: the rows of 08Extend (bytes, one `SUBKMER,m|l|r,EXTENSION` row per line) -> the rows of 09ExtendAgain"""
        text = bytes(text)
        off, n_rows = self._row_offsets(text)
        cap = len(text) + 64 * n_rows + 64
        return self._host_text_call("rfx_ext2_text", [cap], lambda o, c, ln: self.L.rfx_ext2_text(
            self.ctx, text, off.ctypes.data, n_rows, int(P), C.byref(params), o[0].ctypes.data, c[0], C.addressof(ln[0])))[0]

    # ------------------------------------------------ f-4: contig RC de-duplication
    def dedup_contigs(self, contigs, min_contig=500):
        """rfx_dedup_contigs (P/ReflexivDSDynamicKmerDedup.java :138-339) on a list of contig strings (ids = positions) ->
        (survivors: list of strings, text, [contigs after round 1, 2, 3])"""
        off = np.zeros(len(contigs) + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in contigs])
        bases = np.frombuffer("".join(contigs).encode(), np.uint8) if off[-1] else np.zeros(1, np.uint8)
        n = len(contigs)
        ob = np.empty(int(2 * off[-1]) + 4096, np.uint8)
        oo = np.empty(n + 2, np.int64)
        m, tl = C.c_int64(0), C.c_int64(0)
        rn = (C.c_int64 * 3)()
        tcap = int(2 * off[-1]) + 64 * (n + 2) + 4096
        tb = np.empty(tcap, np.uint8)
        t0 = time.perf_counter()
        st = self.L.rfx_dedup_contigs(self.ctx, _p(bases), _p(off), C.c_int64(n), min_contig, _p(ob), C.c_int64(len(ob)), _p(oo),
                                      C.c_int64(n + 1), C.byref(m), _p(tb), C.c_int64(tcap), C.byref(tl), rn)
        self.last_call_ms = (time.perf_counter() - t0) * 1e3        # inside the C ABI: what a C / Java host pays
        self._check(st, "rfx_dedup_contigs")
        k = int(m.value)
        surv = [bytes(ob[oo[i]:oo[i + 1]]).decode() for i in range(k)]
        return surv, bytes(tb[:tl.value]).decode(), [int(x) for x in rn]

    def dedup_contig_text(self, text: str, min_contig=500):
        """rfx_dedup_contig_text: the path's contig text -> (de-duplicated text, contigs, [after round 1, 2, 3])"""
        src = text.encode()
        cap = len(src) + 4096
        out = np.empty(cap, np.uint8)
        ln, nc = C.c_int64(0), C.c_int64(0)
        rn = (C.c_int64 * 3)()
        self._check(self.L.rfx_dedup_contig_text(self.ctx, src, C.c_int64(len(src)), min_contig, _p(out), C.c_int64(cap), C.byref(ln),
                                                 C.byref(nc), rn), "rfx_dedup_contig_text")
        return bytes(out[:ln.value]).decode(), int(nc.value), [int(x) for x in rn]

    # ---- the same on a packed contig set that stays in HBM (rfx_dev_contigs_*, rfx_dev_dedup_contigs)
    def contigs_pack(self, contigs, out: "ContigsPacked" = None) -> "ContigsPacked":
        """rfx_dev_contigs_pack: a list of contig strings -> a packed set in HBM (a letter that is not ACGT is code 3)"""
        n = len(contigs)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in contigs])
        bases = np.frombuffer("".join(contigs).encode(), np.uint8) if off[-1] else np.zeros(1, np.uint8)
        out = out or ContigsPacked(n, n + int(off[-1]) // 32)
        return self._grow_call(self.L.rfx_dev_contigs_pack, "rfx_dev_contigs_pack", out,
                                      lambda co: (bases.ctypes.data, off.ctypes.data, n, C.byref(co)))

    def contigs_unpack(self, d: "ContigsPacked"):
        """rfx_dev_contigs_unpack: a packed set -> the list of contig strings"""
        ci = d._c()
        cap_b, cap_n = 32 * d.words + 64, d.n
        ob, oo, m = np.empty(cap_b, np.uint8), np.empty(cap_n + 1, np.int64), C.c_int64(0)
        t0 = time.perf_counter()
        st = self.L.rfx_dev_contigs_unpack(self.ctx, C.byref(ci), ob.ctypes.data, cap_b, oo.ctypes.data, cap_n, C.addressof(m))
        self.last_call_ms = (time.perf_counter() - t0) * 1e3
        self._check(st, "rfx_dev_contigs_unpack")
        return [bytes(ob[oo[i]:oo[i + 1]]).decode() for i in range(int(m.value))]

    def contigs_from_text_dev(self, d_text, length: int = None, out: "ContigsPacked" = None) -> "ContigsPacked":
        """rfx_dev_contigs_from_text: the contig text the path writes (torch uint8 tensor in HBM) -> a packed set"""
        length = int(d_text.numel()) if length is None else int(length)
        out = out or ContigsPacked(max(16, length // 64), length // 32 + max(16, length // 64))
        return self._grow_call(self.L.rfx_dev_contigs_from_text, "rfx_dev_contigs_from_text", out,
                                      lambda co: (d_text.data_ptr(), length, C.byref(co)))

    def contigs_to_text_dev(self, d: "ContigsPacked", min_contig=500, d_text=None):
        """rfx_dev_contigs_to_text -> (torch uint8 tensor in HBM holding ">Contig-<len>-<idx>\n" + sequence, its length, the
        contigs written)"""
        import torch
        ci = d._c()
        nc = C.c_int64(0)
        if d_text is None:
            d_text = torch.empty(max(1, 64 * d.n + 33 * d.words + 64), dtype=torch.uint8, device=d.word_off.device)
        d_text, n = self._dev_text_call("rfx_dev_contigs_to_text", d_text, lambda t, ln: self.L.rfx_dev_contigs_to_text(
            self.ctx, C.byref(ci), min_contig, t.data_ptr(), int(t.numel()), C.addressof(ln), C.addressof(nc)))
        return d_text, n, int(nc.value)

    def dedup_dev(self, d: "ContigsPacked", out: "ContigsPacked" = None):
        """rfx_dev_dedup_contigs: the three rounds, packed in, packed out -> (ContigsPacked, [contigs after round 1, 2, 3])"""
        ci = d._c()
        rn = (C.c_int64 * 3)()
        out = self._grow_call(self.L.rfx_dev_dedup_contigs, "rfx_dev_dedup_contigs", out or ContigsPacked(d.n, d.words),
                                     lambda co: (C.byref(ci), C.byref(co), C.addressof(rn)))
        return out, [int(x) for x in rn]

    # ------------------------------------------------ several GPUs: the RCCL exchange behind the C ABI
    @staticmethod
    def comm_unique_id() -> bytes:
        """rank 0: the 128-byte RCCL id every rank passes to comm_init (hand it round with whatever the host has)"""
        buf = (C.c_uint8 * 128)()
        st = _lib.lib().rfx_comm_unique_id(buf)
        if st != RFX_OK:
            raise RfxError(st, "rfx_comm_unique_id", "RCCL is not available")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """collective: -> this rank's communicator handle (kept by the object; comm_destroy / close free it)"""
        assert len(unique_id) == 128
        h = C.c_void_p(0)
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self.L.rfx_comm_init(self.ctx, buf, rank, world, C.byref(h)), "rfx_comm_init")
        self.comm = h
        self.comm_rank, self.comm_world = rank, world
        return h

    def trim(self):
        """rfx_ctx_trim: the context's grow-only workspaces back to the driver"""
        self._check(self.L.rfx_ctx_trim(self.ctx), "rfx_ctx_trim")

    def workspace_bytes(self) -> int:
        return int(self.L.rfx_ctx_workspace_bytes(self.ctx))

    def comm_destroy(self):
        if getattr(self, "comm", None):
            self.L.rfx_comm_destroy(self.comm)
            self.comm = None

    def comm_all_reduce(self, vals, op: str = "sum"):
        a = (C.c_int64 * len(vals))(*[int(v) for v in vals])
        self._check(self.L.rfx_comm_all_reduce_i64(self.comm, a, len(vals), 0 if op == "sum" else 1), "rfx_comm_all_reduce_i64")
        return [int(x) for x in a]

    def sharded_count_dev(self, d_words: int, n_reads: int, words_per_read: int, read_len: int, k: int, d_out_keys: int,
                          d_out_counts: int, cap: int, min_cov=2, max_cov=10_000_000, twin=TWIN_DS, generations=4,
                          front_clip=0, end_clip=0, d_read_len: int = 0):
        """collective (rfx_dev_sharded_count): this rank's reads -> its ascending shard; -> (m, [instances, distinct,
        survivors] over all ranks).  RfxError(RFX_E_CAP) carries the needed capacity in .need."""
        n = C.c_int64(0)
        tot = (C.c_int64 * 3)()
        st = self.L.rfx_dev_sharded_count(self.ctx, self.comm, C.c_void_p(d_words), C.c_void_p(d_read_len), C.c_int64(n_reads), words_per_read,
                                          read_len, k, front_clip, end_clip, generations, min_cov, max_cov, twin,
                                          C.c_void_p(d_out_keys), C.c_void_p(d_out_counts), C.c_int64(cap), C.byref(n), tot)
        if st == RFX_E_CAP:
            e = RfxError(st, "rfx_dev_sharded_count", f"needs room for {n.value} survivors, cap is {cap}")
            e.need = int(n.value)
            raise e
        self._check(st, "rfx_dev_sharded_count")
        return int(n.value), [int(x) for x in tot]

    def sharded_assemble_dev(self, d_keys: int, d_counts: int, n: int, prm: Params, gather_below: int = -1, text_cap: int = None):
        """collective (rfx_dev_sharded_assemble): this rank's shard of the filtered (k-mer, count) list in HBM -> (text, n_contigs,
        trace) on rank 0 ("" elsewhere), the extend stage range-sharded over the ranks while the record set has more than
        gather_below records (-1: the library's default, 0: to the end of the loop)"""
        trace = np.zeros(prm.max_iter + 8, np.int64)
        cap = (1 << 20) + 64 * max(n, 1) if text_cap is None else int(text_cap)
        self.text_retries = 0
        while True:
            buf = np.empty(max(cap, 1), np.uint8)
            ln, nc, ntr = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            st = self.L.rfx_dev_sharded_assemble(self.ctx, self.comm, C.c_void_p(d_keys), C.c_void_p(d_counts), C.c_int64(n), C.byref(prm),
                                                 C.c_int64(gather_below), _p(buf), C.c_int64(cap), C.byref(ln), C.byref(nc), _p(trace),
                                                 C.c_int64(len(trace)), C.byref(ntr))
            if st == RFX_E_CAP and ln.value > cap:
                cap = int(ln.value)
                self.text_retries += 1
                continue
            self._check(st, "rfx_dev_sharded_assemble")
            return bytes(buf[:ln.value]).decode(), int(nc.value), [int(x) for x in trace[:ntr.value]]

    def sharded_assemble_reads(self, bases, read_off, prm: Params, generations: int = 4, text_cap: int = None, gather_below: int = -1):
        """collective (rfx_sharded_assemble_reads): this rank's ASCII reads -> (text, n_contigs, trace, totals); text on rank 0.
        k = 21..31 and 33..124, not 64 or 96 (the latter as assemble_reads takes it).
        A text buffer that is too short on rank 0 is RFX_E_CAP on EVERY rank (with the length rank 0 needs), so the retry below
        re-enters the collective on all ranks together; text_cap forces a first size (tests)."""
        bases = np.ascontiguousarray(bases, np.uint8)
        read_off = np.ascontiguousarray(read_off, np.int64)
        n_reads = len(read_off) - 1
        trace = np.zeros(prm.max_iter + 8, np.int64)
        tot = (C.c_int64 * 3)()
        cap = 3 * len(bases) + (1 << 20) if text_cap is None else int(text_cap)
        self.text_retries = 0
        while True:
            buf = np.empty(max(cap, 1), np.uint8)
            ln, nc, ntr = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            st = self.L.rfx_sharded_assemble_reads(self.ctx, self.comm, _p(bases), _p(read_off), C.c_int64(n_reads), C.byref(prm),
                                                   generations, C.c_int64(gather_below), _p(buf), C.c_int64(cap), C.byref(ln), C.byref(nc), _p(trace),
                                                   C.c_int64(len(trace)), C.byref(ntr), tot)
            if st == RFX_E_CAP and ln.value > cap:
                cap = int(ln.value)
                self.text_retries += 1
                continue
            self._check(st, "rfx_sharded_assemble_reads")
            return (bytes(buf[:ln.value]).decode(), int(nc.value), [int(x) for x in trace[:ntr.value]], [int(x) for x in tot])

    def comm_bytes_bucketed(self) -> int:
        return int(self.L.rfx_comm_last_bytes_bucketed(self.comm))

    def gather_shards_dev(self, d_keys: int, d_counts: int, n: int, key_words: int, count_bytes: int, root: int,
                          d_out_keys: int, d_out_counts: int, cap: int) -> int:
        m = C.c_int64(0)
        st = self.L.rfx_dev_gather_shards(self.ctx, self.comm, C.c_void_p(d_keys), C.c_void_p(d_counts), C.c_int64(n), key_words,
                                          count_bytes, root, C.c_void_p(d_out_keys), C.c_void_p(d_out_counts), C.c_int64(cap),
                                          C.byref(m))
        if st == RFX_E_CAP:
            e = RfxError(st, "rfx_dev_gather_shards", f"needs room for {m.value} entries, cap is {cap}")
            e.need = int(m.value)
            raise e
        self._check(st, "rfx_dev_gather_shards")
        return int(m.value)

    def count_timing(self):
        """Per-kernel-family HIP-event timing of the last count call: {name: (ms, launches)}; the "stat_*" entries carry
        the leaf tables' statistics in `launches` (leaves, table passes, passes abandoned on overflow) and the last level's
        (records of children that outgrew their regions and were moved, sweeps given up for the exact form, sweeps that ran and stood);
        `stat_records`: super-k-mer records level 1's one sweep wrote (absent when the two-pass form ran);
        `stat_l1_void_rounds`: level-1 sweeps given up because a round put more into one bin than the two extents in hand take
        (absent otherwise; a sweep whose region ran out does not count here)."""
        out = {}
        for name in ("hist1", "part1", "hist2", "part2", "hist3", "part3", "leaf", "sort", "extract_w", "count_w",
                     "pair_hist", "pair_part", "stat_leaves", "stat_passes", "stat_overflows", "stat_l2_spilled", "stat_l2_void", "stat_l2_sweeps",
                     "stat_records", "stat_l1_void_rounds"):
            ms, ln = C.c_float(0), C.c_int64(0)
            if self.L.rfx_last_count_timing(self.ctx, name.encode(), C.byref(ms), C.byref(ln)) == RFX_OK:
                out[name] = (float(ms.value), int(ln.value))
        return out
