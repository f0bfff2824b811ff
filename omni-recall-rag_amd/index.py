"""RecallIndex: a thin Python handle over the C ABI (include/omnirecall_hip.h),
used by the tests, bench.py and the sharded front-end.  It adds no arithmetic:
every score comes out of libomnirecall_hip.so."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N

CAND_DTYPE = np.dtype([("approx_score", "<f8"), ("dot", "<f8"), ("norm_b", "<f8"), ("created_ticks", "<i8"),
                       ("row_id", "<i8"), ("order_key", "<i8"), ("matches", "<i4"), ("flags", "<i4")])
assert CAND_DTYPE.itemsize == C.sizeof(N.OrrCandidate) == 56


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _ptr(x) -> Optional[int]:
    """Raw address of a numpy array or torch tensor (host or device).  The library reads device memory on its own
    streams (include/omnirecall_hip.h, conventions): whatever torch still has queued for a CUDA tensor is waited for."""
    if x is None:
        return None
    if _is_torch(x):
        assert x.is_contiguous()
        if x.is_cuda:
            import torch
            torch.cuda.current_stream(x.device).synchronize()
        return x.data_ptr()
    assert x.flags["C_CONTIGUOUS"]
    return x.ctypes.data


class PackedTerms:
    """(terms_utf8, term_off, query_term_off) already in the ABI's form; accepted wherever a list of
    per-query term lists is (saves re-packing the same batch for several calls).  Indexing gives one
    query's terms as a list of bytes, like the list form."""

    def __init__(self, arrays):
        self.arrays = tuple(arrays)

    def __len__(self):
        return int(self.arrays[2].shape[0]) - 1

    def __getitem__(self, b: int):
        pool, toff, qoff = self.arrays
        return [bytes(pool[int(toff[i]):int(toff[i + 1])]) for i in range(int(qoff[b]), int(qoff[b + 1]))]

    def __iter__(self):
        return (self[b] for b in range(len(self)))


def pack_terms(queries_terms) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """[[term bytes]] per query -> (terms_utf8, term_off, query_term_off) of the ABI."""
    if isinstance(queries_terms, PackedTerms):
        return queries_terms.arrays
    flat = [bytes(t) for terms in queries_terms for t in terms]
    pool_arr = np.frombuffer(b"".join(flat) + b"\0", dtype=np.uint8).copy()
    term_off = np.zeros(len(flat) + 1, dtype=np.uint32)
    if flat:
        np.cumsum(np.fromiter(map(len, flat), dtype=np.int64, count=len(flat)), out=term_off[1:])
    qoff = np.zeros(len(queries_terms) + 1, dtype=np.uint32)
    if len(queries_terms):
        np.cumsum(np.fromiter(map(len, queries_terms), dtype=np.int64, count=len(queries_terms)), out=qoff[1:])
    return pool_arr, term_off, qoff


def pack_contents(contents: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(contents) + 1, dtype=np.uint64)
    if len(contents):
        off[1:] = np.cumsum([len(c) for c in contents], dtype=np.uint64)
    pool = np.frombuffer(b"".join(bytes(c) for c in contents) + b"\0", dtype=np.uint8).copy()
    return pool, off


def _near_args(probes, mode: str, device_ok: bool):
    """(n_probes, dim, array kept alive, mode) of a cosine scope's probes: [n, dim] float32, numpy or (device_ok) a torch tensor;
    None or an empty list is no probes."""
    modes = {"all": N.ORR_NEAR_ALL, "any": N.ORR_NEAR_ANY}
    if mode not in modes:
        raise ValueError('mode: "all" or "any"')
    if probes is None:
        return 0, 0, None, modes[mode]
    if _is_torch(probes) and device_ok:
        import torch
        p = probes.to(torch.float32).contiguous()
    else:
        p = np.ascontiguousarray(probes, dtype=np.float32)
    if p.ndim == 1:
        p = p.reshape(1, -1) if p.shape[0] else p.reshape(0, 0)
    if p.ndim != 2:
        raise ValueError("probes: [n_probes, dim]")
    return int(p.shape[0]), int(p.shape[1]), p, modes[mode]


RANGE_HIT_DTYPE = np.dtype([("row_id", "<i8"), ("order_key", "<i8"), ("cosine", "<f8")])
assert RANGE_HIT_DTYPE.itemsize == 24


def _range_cosine(call, handle, qvecs, min_cosine, max_hits: int, within, device_ok: bool):
    """orr_search_range_cosine / orr_cluster_search_range_cosine through `call`.  Returns (row_ids, order_keys, cosines, totals):
    three lists of per-query arrays, best hit first, and totals [B] int64, the exact number of hits of each query.  Over the
    pair limit the OrrError (code ORR_ELIMIT) carries `totals`: every query's upper bound."""
    t = np.ascontiguousarray(min_cosine, dtype=np.float64).reshape(-1)
    B = int(t.shape[0])
    if qvecs is None:
        dim, q = 0, None
    else:
        if _is_torch(qvecs) and device_ok:
            import torch
            q = qvecs.to(torch.float32).contiguous()
        else:
            q = np.ascontiguousarray(qvecs, dtype=np.float32)
        if q.ndim == 1 and B == 1:
            q = q.reshape(1, -1)
        if q.ndim != 2 or int(q.shape[0]) != B:
            raise ValueError(f"qvecs: [{B}, dim] for {B} thresholds")
        dim = int(q.shape[1])
    k = int(max_hits)
    hits = np.zeros((B, max(k, 0)), dtype=RANGE_HIT_DTYPE)
    n = np.zeros(max(B, 1), dtype=np.int32)
    totals = np.zeros(max(B, 1), dtype=np.int64)
    status = call(handle, B, dim, _ptr(q) if dim else None, _ptr(t) if B else None, within._h if within is not None else None, k,
                  _ptr(hits) if k > 0 and B else None, _ptr(n), _ptr(totals))
    totals = totals[:B]
    if status != N.ORR_OK:
        try:
            N.check(status)
        except N.OrrError as e:
            e.totals = totals
            raise
    rows = [hits[b, :n[b]]["row_id"].copy() for b in range(B)]
    keys = [hits[b, :n[b]]["order_key"].copy() for b in range(B)]
    cos = [hits[b, :n[b]]["cosine"].copy() for b in range(B)]
    return rows, keys, cos, totals


class RecallScope:
    """A scope handle (orr_scope): a set of ROWS of one sealed shard, resolved once and resident on its device.  It follows
    its rows through delete_rows, compact and insert_rows of the shard; rows inserted later are in no scope until add_ids
    names them.  Made by RecallIndex.scope / scope_ticks / scope_terms / scope_near; close it before or after its index (after: only the host part is
    left to free)."""

    def __init__(self, handle, index: "RecallIndex"):
        self._h = handle
        self._index = index                  # keeps the index object alive

    def close(self) -> None:
        if getattr(self, "_h", None):
            N.hip.orr_scope_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self) -> int:
        """orr_scope_rows: live rows in the scope now; -1 once its index was destroyed."""
        return int(N.hip.orr_scope_rows(self._h))

    def row_ids(self) -> np.ndarray:
        """orr_scope_row_ids: the ids of the scope's live rows, in candidate order."""
        n = C.c_int64(0)
        out = np.zeros(max(self.rows, 0), dtype=np.int64)
        N.check(N.hip.orr_scope_row_ids(self._h, int(out.shape[0]), _ptr(out) if out.shape[0] else None, C.cast(C.byref(n), C.c_void_p)))
        return out[:int(n.value)]

    def centroid(self, sums: bool = False):
        """orr_scope_centroid: (centroid [dim] float32, used) -- the mean of the scope's rows that have a vector, all of them
        one group under orr_keys_centroids' rule.  sums=True: (centroid, sum [dim] float64, used)."""
        dim = int(self._index.dim)
        cent = np.zeros(dim, dtype=np.float32)
        S = np.zeros(dim, dtype=np.float64)
        used = C.c_int64(0)
        N.check(N.hip.orr_scope_centroid(self._h, dim, _ptr(cent) if dim else None, _ptr(S) if dim else None, C.cast(C.byref(used), C.c_void_p)))
        return (cent, S, int(used.value)) if sums else (cent, int(used.value))

    def add_ids(self, row_ids) -> int:
        """orr_scope_add_ids: the live rows that carry these ids join the scope.  Returns how many were not in it before."""
        ids = row_ids if _is_torch(row_ids) else np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        n_ids = int(ids.shape[0])
        added = C.c_int64(0)
        N.check(N.hip.orr_scope_add_ids(self._h, n_ids, _ptr(ids) if n_ids else None, C.cast(C.byref(added), C.c_void_p)))
        return int(added.value)

    def _combine(self, op: int, other: "RecallScope") -> "RecallScope":
        N.check(N.hip.orr_scope_combine(self._h, op, other._h))
        return self

    def and_(self, other: "RecallScope") -> "RecallScope":
        """self = self AND other, in place."""
        return self._combine(N.ORR_SCOPE_AND, other)

    def or_(self, other: "RecallScope") -> "RecallScope":
        """self = self OR other, in place."""
        return self._combine(N.ORR_SCOPE_OR, other)

    def andnot(self, other: "RecallScope") -> "RecallScope":
        """self = self AND NOT other, in place."""
        return self._combine(N.ORR_SCOPE_ANDNOT, other)


class RecallKeys:
    """Row keys (orr_keys): one int64 key per row of one sealed shard, resident on its device; KEY_NONE means "no key".  A key
    is whatever the host groups by, typically a document number.  The column follows its rows through compact and insert_rows
    of the shard; rows inserted later read KEY_NONE until `set` names them.  Made by RecallIndex.keys; close it before or
    after its index (after: only the host part is left to free)."""

    KEY_NONE = N.ORR_KEY_NONE

    def __init__(self, handle, index: "RecallIndex"):
        self._h = handle
        self._index = index                  # keeps the index object alive

    def close(self) -> None:
        if getattr(self, "_h", None):
            N.hip.orr_keys_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _pairs(row_ids, keys):
        if _is_torch(row_ids) != _is_torch(keys):
            raise ValueError("row_ids and keys live in the same memory: both numpy or both torch")
        if _is_torch(row_ids):                           # (the library reads raw int64: no other dtype, layout or mixed placement)
            import torch
            if row_ids.device != keys.device:
                raise ValueError("row_ids and keys live in the same memory: both on the host or both on one device")
            row_ids = row_ids.to(torch.int64).reshape(-1).contiguous()
            keys = keys.to(torch.int64).reshape(-1).contiguous()
        else:
            row_ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
            keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        if int(row_ids.shape[0]) != int(keys.shape[0]):
            raise ValueError("one key per row id")
        return row_ids, keys, int(row_ids.shape[0])

    def set(self, row_ids, keys) -> int:
        """orr_keys_set: keys[i] is stored at the live rows that carry row_ids[i] (numpy or torch, both in the same memory).
        Returns how many entries named a live row.  An id listed twice with different keys gets one of them."""
        ids, ks, n = self._pairs(row_ids, keys)
        done = C.c_int64(0)
        N.check(N.hip.orr_keys_set(self._h, n, _ptr(ids) if n else None, _ptr(ks) if n else None, C.cast(C.byref(done), C.c_void_p)))
        return int(done.value)

    def get(self, row_ids) -> np.ndarray:
        """orr_keys_get: the keys of these row ids (host); an unknown or deleted id reads KEY_NONE."""
        ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        out = np.full(ids.shape[0], N.ORR_KEY_NONE, dtype=np.int64)
        n = int(ids.shape[0])
        N.check(N.hip.orr_keys_get(self._h, n, _ptr(ids) if n else None, _ptr(out) if n else None))
        return out

    @property
    def rows(self) -> int:
        """orr_keys_rows: live rows whose key is not KEY_NONE; -1 once the index was destroyed."""
        return int(N.hip.orr_keys_rows(self._h))

    def groups(self, within: Optional["RecallScope"] = None, cap: Optional[int] = None):
        """orr_keys_groups: (keys, rows) -- the distinct keys other than KEY_NONE among the live rows (of `within`), ascending,
        and how many rows carry each.  cap: at most this many entries (the first ones); None: all of them."""
        wh = within._h if within is not None else None
        n, total = C.c_int64(0), C.c_int64(0)
        pn, pt = C.cast(C.byref(n), C.c_void_p), C.cast(C.byref(total), C.c_void_p)
        if cap is None:
            N.check(N.hip.orr_keys_groups(self._h, wh, 0, None, None, pn, pt))
            cap = int(total.value)
        keys = np.zeros(int(cap), dtype=np.int64)
        rows = np.zeros(int(cap), dtype=np.int64)
        N.check(N.hip.orr_keys_groups(self._h, wh, int(cap), _ptr(keys) if cap else None, _ptr(rows) if cap else None, pn, pt))
        return keys[:int(n.value)], rows[:int(n.value)]

    def centroids(self, keys, within: Optional["RecallScope"] = None, sums: bool = False):
        """orr_keys_centroids: (centroids [n, dim] float32, used [n] int64) -- per listed key the mean of its live rows (of
        `within`) that have a vector (normB > 0), summed in fp64 in the blocked order the header states; a key without such a
        row gives zeros and used 0.  sums=True: (centroids, sums [n, dim] float64, used)."""
        ks = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        n, dim = int(ks.shape[0]), int(self._index.dim)
        cent = np.zeros((n, dim), dtype=np.float32)
        S = np.zeros((n, dim), dtype=np.float64) if sums else None
        used = np.zeros(n, dtype=np.int64)
        N.check(N.hip.orr_keys_centroids(self._h, within._h if within is not None else None, n, _ptr(ks) if n else None, dim,
                                         _ptr(cent) if cent.size else None, _ptr(S) if sums and S.size else None, _ptr(used) if n else None))
        return (cent, S, used) if sums else (cent, used)

    def centroid_index(self, within: Optional["RecallScope"] = None) -> "RecallIndex":
        """orr_keys_centroid_index: a sealed, owned RecallIndex with one row per key that has a row with a vector (of `within`):
        the key's centroid (centroids' bits) as its embedding, the key as its row id, the ticks of its newest such row, no
        content.  A snapshot, independent of this column and its index; `docs` and `skipped` (keys dropped for having no row
        with a vector) are attributes of the result."""
        h = C.c_void_p()
        docs, skipped = C.c_int64(0), C.c_int64(0)
        N.check(N.hip.orr_keys_centroid_index(self._h, within._h if within is not None else None, C.byref(h),
                                              C.cast(C.byref(docs), C.c_void_p), C.cast(C.byref(skipped), C.c_void_p)))
        out = RecallIndex.__new__(RecallIndex)
        out._h = h
        out.dim = int(N.hip.orr_index_dim(h))
        out.row_base = 0
        out.docs, out.skipped = int(docs.value), int(skipped.value)
        return out


class _BorrowedKeys(RecallKeys):
    """A shard's part of a RecallClusterKeys: usable like a RecallKeys (get, rows, RecallIndex.search_per_key on the shard),
    never destroyed through this object; it ends with its cluster keys."""

    def close(self) -> None:
        self._h = None


class RecallClusterKeys:
    """Row keys over a cluster (orr_cluster_keys): one RecallKeys per shard behind one handle.  It follows its rows through
    delete_rows on a shard, RecallCluster.compact and insert_rows; rows inserted later read KEY_NONE until `set` names them.
    Made by RecallCluster.keys; close it before or after its cluster (after: only the host part is left to free)."""

    KEY_NONE = N.ORR_KEY_NONE

    def __init__(self, handle, cluster: "RecallCluster"):
        self._h = handle
        self._cluster = cluster              # keeps the cluster object alive
        self._parts = []

    def close(self) -> None:
        if getattr(self, "_h", None):
            for part in self._parts:
                part.close()
            self._parts = []
            N.hip.orr_cluster_keys_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _pairs(row_ids, keys):
        ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        ks = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        if int(ids.shape[0]) != int(ks.shape[0]):
            raise ValueError("one key per row id")
        return ids, ks, int(ids.shape[0])

    def set(self, row_ids, keys) -> int:
        """orr_cluster_keys_set: keys[i] is stored at the live rows that carry row_ids[i], on every shard (numpy, host memory).
        Returns the SUM of the shards' counts: an id that is live on two shards counts twice."""
        ids, ks, n = self._pairs(row_ids, keys)
        done = C.c_int64(0)
        N.check(N.hip.orr_cluster_keys_set(self._h, n, _ptr(ids) if n else None, _ptr(ks) if n else None, C.cast(C.byref(done), C.c_void_p)))
        return int(done.value)

    def get(self, row_ids) -> np.ndarray:
        """orr_cluster_keys_get: the keys of these row ids (host): per id the lowest shard's key that is not KEY_NONE."""
        ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        out = np.full(ids.shape[0], N.ORR_KEY_NONE, dtype=np.int64)
        n = int(ids.shape[0])
        N.check(N.hip.orr_cluster_keys_get(self._h, n, _ptr(ids) if n else None, _ptr(out) if n else None))
        return out

    @property
    def rows(self) -> int:
        """orr_cluster_keys_rows: live rows whose key is not KEY_NONE, over all shards; -1 once it is orphaned."""
        return int(N.hip.orr_cluster_keys_rows(self._h))

    def groups(self, within: Optional["RecallClusterScope"] = None, cap: Optional[int] = None):
        """orr_cluster_keys_groups: (keys, rows) -- RecallKeys.groups of one index holding all the cluster's rows: the distinct
        keys other than KEY_NONE among the live rows (of `within`), ascending, and how many rows carry each, over all shards."""
        wh = within._h if within is not None else None
        n, total = C.c_int64(0), C.c_int64(0)
        pn, pt = C.cast(C.byref(n), C.c_void_p), C.cast(C.byref(total), C.c_void_p)
        if cap is None:
            N.check(N.hip.orr_cluster_keys_groups(self._h, wh, 0, None, None, pn, pt))
            cap = int(total.value)
        keys = np.zeros(int(cap), dtype=np.int64)
        rows = np.zeros(int(cap), dtype=np.int64)
        N.check(N.hip.orr_cluster_keys_groups(self._h, wh, int(cap), _ptr(keys) if cap else None, _ptr(rows) if cap else None, pn, pt))
        return keys[:int(n.value)], rows[:int(n.value)]

    def centroids(self, keys, within: Optional["RecallClusterScope"] = None, sums: bool = False):
        """orr_cluster_keys_centroids: (centroids [n, dim] float32, used [n] int64) -- RecallKeys.centroids of one index holding
        all the cluster's rows in the global candidate order, bit for bit: a key's blocks of 256 are counted from its first
        member on any shard.  sums=True: (centroids, sums [n, dim] float64, used)."""
        ks = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        n, dim = int(ks.shape[0]), int(self._cluster.dim)
        cent = np.zeros((n, dim), dtype=np.float32)
        S = np.zeros((n, dim), dtype=np.float64) if sums else None
        used = np.zeros(n, dtype=np.int64)
        N.check(N.hip.orr_cluster_keys_centroids(self._h, within._h if within is not None else None, n, _ptr(ks) if n else None, dim,
                                                 _ptr(cent) if cent.size else None, _ptr(S) if sums and S.size else None, _ptr(used) if n else None))
        return (cent, S, used) if sums else (cent, used)

    def shard(self, i: int) -> RecallKeys:
        """orr_cluster_keys_shard: shard i's part, borrowed."""
        p = N.hip.orr_cluster_keys_shard(self._h, int(i))
        if not p:
            N.check(N.ORR_EINVAL)
        part = _BorrowedKeys(C.c_void_p(p), self)
        self._parts.append(part)
        return part


class _BorrowedScope(RecallScope):
    """A shard's part of a RecallClusterScope: usable like a RecallScope (rows, row_ids, RecallIndex.search_shard_in_scope),
    never destroyed through this object; it ends with its cluster scope."""

    def close(self) -> None:
        self._h = None


class RecallClusterScope:
    """A cluster scope handle (orr_cluster_scope): a set of ROWS of one sealed cluster, held as one scope per shard.  Every
    rule of RecallScope holds per shard; it follows its rows through delete_rows on a shard, RecallCluster.compact and
    insert_rows.  Made by RecallCluster.scope / scope_ticks / scope_terms; close it before or after its cluster (after: only
    the host part is left to free)."""

    def __init__(self, handle, cluster: "RecallCluster"):
        self._h = handle
        self._cluster = cluster              # keeps the cluster object alive
        self._parts = []

    def close(self) -> None:
        if getattr(self, "_h", None):
            for part in self._parts:
                part.close()
            self._parts = []
            N.hip.orr_cluster_scope_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self) -> int:
        """orr_cluster_scope_rows: live rows in the scope now, over all shards; -1 once it is orphaned."""
        return int(N.hip.orr_cluster_scope_rows(self._h))

    def row_ids(self) -> np.ndarray:
        """orr_cluster_scope_row_ids: the ids of the scope's live rows in the global candidate order."""
        n = C.c_int64(0)
        out = np.zeros(max(self.rows, 0), dtype=np.int64)
        N.check(N.hip.orr_cluster_scope_row_ids(self._h, int(out.shape[0]), _ptr(out) if out.shape[0] else None, C.cast(C.byref(n), C.c_void_p)))
        return out[:int(n.value)]

    def centroid(self, sums: bool = False):
        """orr_cluster_scope_centroid: (centroid [dim] float32, used) -- RecallScope.centroid of one index holding all the
        cluster's rows in the global candidate order, bit for bit.  sums=True: (centroid, sum [dim] float64, used)."""
        dim = int(self._cluster.dim)
        cent = np.zeros(dim, dtype=np.float32)
        S = np.zeros(dim, dtype=np.float64)
        used = C.c_int64(0)
        N.check(N.hip.orr_cluster_scope_centroid(self._h, dim, _ptr(cent) if dim else None, _ptr(S) if dim else None, C.cast(C.byref(used), C.c_void_p)))
        return (cent, S, int(used.value)) if sums else (cent, int(used.value))

    def add_ids(self, row_ids) -> int:
        """orr_cluster_scope_add_ids: the live rows that carry these ids (numpy, host memory) join the scope on every shard.
        Returns how many were not in it before."""
        ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        n_ids = int(ids.shape[0])
        added = C.c_int64(0)
        N.check(N.hip.orr_cluster_scope_add_ids(self._h, n_ids, _ptr(ids) if n_ids else None, C.cast(C.byref(added), C.c_void_p)))
        return int(added.value)

    def _combine(self, op: int, other: "RecallClusterScope") -> "RecallClusterScope":
        N.check(N.hip.orr_cluster_scope_combine(self._h, op, other._h))
        return self

    def and_(self, other: "RecallClusterScope") -> "RecallClusterScope":
        """self = self AND other, in place, on every shard."""
        return self._combine(N.ORR_SCOPE_AND, other)

    def or_(self, other: "RecallClusterScope") -> "RecallClusterScope":
        """self = self OR other, in place, on every shard."""
        return self._combine(N.ORR_SCOPE_OR, other)

    def andnot(self, other: "RecallClusterScope") -> "RecallClusterScope":
        """self = self AND NOT other, in place, on every shard."""
        return self._combine(N.ORR_SCOPE_ANDNOT, other)

    def shard(self, i: int) -> RecallScope:
        """orr_cluster_scope_shard: shard i's part, borrowed."""
        p = N.hip.orr_cluster_scope_shard(self._h, int(i))
        if not p:
            N.check(N.ORR_EINVAL)
        part = _BorrowedScope(C.c_void_p(p), self)
        self._parts.append(part)
        return part


class RecallIndex:
    """One corpus shard resident on one GPU (orr_index)."""

    def __init__(self, dim: int, device: int = 0, capacity_rows: int = 0, row_base: int = 0):
        cfg = N.OrrConfig(C.sizeof(N.OrrConfig), device, dim, 0, capacity_rows, row_base)
        h = C.c_void_p()
        N.check(N.hip.orr_index_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.dim = dim
        self.row_base = row_base

    def close(self) -> None:
        if getattr(self, "_h", None):
            N.hip.orr_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self) -> int:
        return int(N.hip.orr_index_rows(self._h))

    def append(self, emb, created_ticks, content_lower, content_off=None, row_ids=None) -> None:
        """emb: [n, dim] float32 (numpy or torch, host or device) or None for rows without an
        embedding; created_ticks: [n] int64; content_lower: list of lowercased bytes, or a uint8
        pool with content_off [n+1] uint64 (numpy or torch)."""
        if content_off is None:
            content_lower, content_off = pack_contents(content_lower)
        n = int(content_off.shape[0]) - 1
        if not _is_torch(created_ticks):
            created_ticks = np.ascontiguousarray(created_ticks, dtype=np.int64)
        if emb is not None and not _is_torch(emb):
            emb = np.ascontiguousarray(emb, dtype=np.float32)
        if row_ids is not None and not _is_torch(row_ids):
            row_ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        dim = 0 if emb is None else int(emb.shape[1])
        N.check(N.hip.orr_index_append(self._h, n, dim, _ptr(emb), _ptr(created_ticks), _ptr(content_lower),
                                       _ptr(content_off), _ptr(row_ids)))

    def seal(self) -> None:
        N.check(N.hip.orr_index_seal(self._h))

    def delete_rows(self, row_ids) -> int:
        """orr_index_delete_rows: the rows with these ids stop taking part in later searches (no reseal).
        Returns how many rows were newly deleted."""
        ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        done = C.c_int64(0)
        N.check(N.hip.orr_index_delete_rows(self._h, int(ids.shape[0]), _ptr(ids), C.cast(C.byref(done), C.c_void_p)))
        return int(done.value)

    def update_rows(self, row_ids, emb) -> int:
        """orr_index_update_rows: the rows with these ids get new vectors in place (reindex; no reseal).  emb: [n, dim]
        float32 (numpy or torch, host or device), or None: the rows lose their embedding.  Unknown and deleted ids are
        skipped; returns how many rows were written."""
        if not _is_torch(row_ids):
            row_ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        n = int(row_ids.shape[0])
        if emb is not None and not _is_torch(emb):
            emb = np.ascontiguousarray(emb, dtype=np.float32)
        if emb is not None and (emb.ndim != 2 or int(emb.shape[0]) != n):
            raise ValueError(f"update_rows: emb must be [{n}, dim], not {tuple(emb.shape)}")
        dim = 0 if emb is None else int(emb.shape[1])
        done = C.c_int64(0)
        N.check(N.hip.orr_index_update_rows(self._h, n, _ptr(row_ids), dim, _ptr(emb), C.cast(C.byref(done), C.c_void_p)))
        return int(done.value)

    def get_rows(self, row_ids) -> Tuple[np.ndarray, np.ndarray]:
        """orr_index_get_rows: (emb [n, dim] float32, found [n] bool) -- the stored vectors of the live rows with these ids, bit
        for bit; an unknown or deleted id gives zeros and found False, a row without an embedding zeros and found True."""
        ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        n, dim = int(ids.shape[0]), int(self.dim)
        emb = np.zeros((n, dim), dtype=np.float32)
        found = np.zeros(n, dtype=np.uint8)
        N.check(N.hip.orr_index_get_rows(self._h, n, _ptr(ids) if n else None, dim, _ptr(emb) if n else None, _ptr(found) if n else None))
        return emb, found.astype(bool)

    @staticmethod
    def _row_args(emb, created_ticks, content_lower, content_off, row_ids):
        if content_off is None:
            content_lower, content_off = pack_contents(content_lower)
        n = int(content_off.shape[0]) - 1
        if not _is_torch(created_ticks):
            created_ticks = np.ascontiguousarray(created_ticks, dtype=np.int64)
        if emb is not None and not _is_torch(emb):
            emb = np.ascontiguousarray(emb, dtype=np.float32)
        if row_ids is None:
            raise ValueError("insert_rows: row_ids are required")
        if not _is_torch(row_ids):
            row_ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        if int(created_ticks.shape[0]) != n or int(row_ids.shape[0]) != n or (emb is not None and (emb.ndim != 2 or int(emb.shape[0]) != n)):
            raise ValueError(f"insert_rows: {n} rows of content need [{n}] ticks, [{n}] row ids and [{n}, dim] vectors")
        dim = 0 if emb is None else int(emb.shape[1])
        return n, dim, emb, created_ticks, content_lower, content_off, row_ids

    def insert_rows(self, emb, created_ticks, content_lower, content_off=None, row_ids=None) -> int:
        """orr_index_insert_rows: rows into the SEALED shard in place, arguments as append() except that row_ids are
        required.  The shard afterwards is what a seal of (the old rows, then these) would make.  Returns the rows inserted."""
        n, dim, emb, created_ticks, content_lower, content_off, row_ids = self._row_args(emb, created_ticks, content_lower, content_off, row_ids)
        done = C.c_int64(0)
        N.check(N.hip.orr_index_insert_rows(self._h, n, dim, _ptr(emb), _ptr(created_ticks), _ptr(content_lower), _ptr(content_off),
                                            _ptr(row_ids), C.cast(C.byref(done), C.c_void_p)))
        return int(done.value)

    @property
    def live_rows(self) -> int:
        return int(N.hip.orr_index_live_rows(self._h))

    def compact(self) -> int:
        """orr_index_compact: the shard rebuilt in place without its deleted rows.  Returns the rows removed."""
        done = C.c_int64(0)
        N.check(N.hip.orr_index_compact(self._h, C.cast(C.byref(done), C.c_void_p)))
        return int(done.value)

    def save(self, path: str) -> None:
        """orr_index_save: the sealed shard as one binary file."""
        N.check(N.hip.orr_index_save(self._h, path.encode()))

    @classmethod
    def load(cls, path: str, device: int = 0, row_base: int = 0) -> "RecallIndex":
        """orr_index_load: a sealed shard from a file written by save()."""
        cfg = N.OrrConfig(C.sizeof(N.OrrConfig), device, 0, 0, 0, row_base)
        h = C.c_void_p()
        N.check(N.hip.orr_index_load(C.byref(cfg), path.encode(), C.byref(h)))
        self = cls.__new__(cls)
        self._h = h
        self.dim = int(N.hip.orr_index_dim(h))
        self.row_base = row_base
        return self

    @staticmethod
    def _query_args(qvecs, n_queries: int):
        if qvecs is None:
            return 0, None, None
        if not _is_torch(qvecs):
            qvecs = np.ascontiguousarray(qvecs, dtype=np.float32).reshape(n_queries, -1)
        dim = int(qvecs.shape[1])
        return dim, (qvecs if dim > 0 else None), qvecs

    def search(self, qvecs, queries_terms: Sequence[Sequence[bytes]], now_ticks: int, topk: int,
               candidate_limit: int = 300):
        """orr_search_batch.  Returns (rows [B,k] int64, scores [B,k] float64, counts [B] int32)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_search_batch(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks,
                                       int(topk), int(candidate_limit), _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def search_shard(self, qvecs, queries_terms, now_ticks: int, kprime: int, candidate_limit: int, out=None,
                     topk: Optional[int] = None, shard_pass: Optional[int] = None):
        """orr_search_shard (or, with topk / shard_pass given, orr_search_shard_ex: the caller's k and the pass as call
        arguments instead of sticky index options).  Returns a [B, kprime+1] structured array (or fills `out`, which may be
        a torch uint8 tensor on the device with B*(kprime+1)*56 bytes)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        if out is None:
            out = np.zeros((B, kprime + 1), dtype=CAND_DTYPE)
        if topk is None and shard_pass is None:
            N.check(N.hip.orr_search_shard(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks,
                                           int(kprime), int(candidate_limit), _ptr(out)))
        else:
            N.check(N.hip.orr_search_shard_ex(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks,
                                              int(kprime), int(candidate_limit), max(0, int(topk or 0)), int(shard_pass or 0), _ptr(out)))
        return out

    @staticmethod
    def _scope_args(scope_ids, n_queries: int):
        """A scope for the ABI: one flat list of row ids (numpy / torch, host or device) shared by every query, or a sequence
        of n_queries lists, one per query.  Returns (n_ids, ids, offsets or None)."""
        shared = _is_torch(scope_ids) or isinstance(scope_ids, np.ndarray) or \
            (len(scope_ids) == 0 or not hasattr(scope_ids[0], "__len__"))
        if shared:
            ids = scope_ids if _is_torch(scope_ids) else np.ascontiguousarray(scope_ids, dtype=np.int64).reshape(-1)
            if _is_torch(ids):
                ids = ids.reshape(-1)
            return int(ids.shape[0]), ids, None
        if len(scope_ids) != n_queries:
            raise ValueError(f"scope_ids: {len(scope_ids)} lists for {n_queries} queries")
        parts = [p if _is_torch(p) else np.ascontiguousarray(p, dtype=np.int64).reshape(-1) for p in scope_ids]
        off = np.zeros(n_queries + 1, dtype=np.uint64)
        off[1:] = np.cumsum([int(p.shape[0]) for p in parts], dtype=np.uint64)
        if parts and all(_is_torch(p) for p in parts):
            import torch
            ids = torch.cat([p.reshape(-1) for p in parts]).contiguous()
        else:
            parts = [p.cpu().numpy() if _is_torch(p) else p for p in parts]
            ids = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, np.int64), dtype=np.int64)
        return int(ids.shape[0]), ids, off

    def search_scoped(self, qvecs, queries_terms, now_ticks: int, topk: int, scope_ids, candidate_limit: int = 300, scope_off=None):
        """orr_search_batch_scoped: every query ranks only the live rows whose id its scope lists.  scope_ids: one flat list
        (numpy or torch, host or device) shared by all queries, a sequence of per-query lists, or -- with scope_off [B+1] given --
        the flat list the offsets cut.  Returns (rows [B,k] int64, scores [B,k] float64, counts [B] int32)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        if scope_off is None:
            n_ids, ids, off = self._scope_args(scope_ids, B)
        else:
            ids = scope_ids if _is_torch(scope_ids) else np.ascontiguousarray(scope_ids, dtype=np.int64).reshape(-1)
            n_ids, off = int(ids.shape[0]), np.ascontiguousarray(scope_off, dtype=np.uint64)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_search_batch_scoped(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                              int(candidate_limit), n_ids, _ptr(ids) if n_ids else None, _ptr(off),
                                              _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def search_masked(self, qvecs, queries_terms, now_ticks: int, topk: int, scope_ids, candidate_limit: int = 300):
        """orr_search_batch_masked: every query ranks only the live rows whose id the ONE shared scope lists (a flat list,
        numpy or torch, host or device) -- the results of search_scoped with a shared list, through a masked two-stage screen
        that reads the shard once per batch; no limit on the size of the scope.  Returns (rows [B,k] int64, scores [B,k]
        float64, counts [B] int32)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        ids = scope_ids if _is_torch(scope_ids) else np.ascontiguousarray(scope_ids, dtype=np.int64).reshape(-1)
        n_ids = int(ids.shape[0])
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_search_batch_masked(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                              int(candidate_limit), n_ids, _ptr(ids) if n_ids else None,
                                              _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def search_masked_groups(self, qvecs, queries_terms, now_ticks: int, topk: int, group_scopes, query_group,
                             candidate_limit: int = 300, group_off=None):
        """orr_search_batch_masked_groups: query b ranks only the live rows whose id group query_group[b] lists -- for every
        query the result of search_masked with its group's ids as the scope, while the groups' large scopes share ONE
        screening pass over the shard.  group_scopes: a sequence of G id arrays, or -- with group_off [G+1] given -- the flat
        array (numpy or torch, host or device) the offsets cut.  At most 64 groups.  Returns (rows [B,k] int64, scores [B,k]
        float64, counts [B] int32)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        if group_off is None:
            n_ids, ids, off = self._scope_args([g for g in group_scopes], len(group_scopes))
            if off is None:                          # (a sequence without a list in it: no groups at all)
                raise ValueError("group_scopes: a sequence of id arrays, or a flat array with group_off")
        else:
            ids = group_scopes if _is_torch(group_scopes) else np.ascontiguousarray(group_scopes, dtype=np.int64).reshape(-1)
            n_ids, off = int(ids.shape[0]), np.ascontiguousarray(group_off, dtype=np.uint64)
        qg = np.ascontiguousarray(query_group, dtype=np.int32).reshape(-1)
        if qg.shape[0] != B:
            raise ValueError(f"query_group: {qg.shape[0]} entries for {B} queries")
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_search_batch_masked_groups(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                                     int(candidate_limit), int(off.shape[0]) - 1, n_ids, _ptr(ids) if n_ids else None,
                                                     _ptr(off), _ptr(qg), _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def scope(self, row_ids) -> RecallScope:
        """orr_scope_create: the live rows that carry these ids (numpy or torch, host or device), resolved once."""
        ids = row_ids if _is_torch(row_ids) else np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        n_ids = int(ids.shape[0])
        h = C.c_void_p()
        N.check(N.hip.orr_scope_create(self._h, n_ids, _ptr(ids) if n_ids else None, C.byref(h)))
        return RecallScope(h, self)

    def scope_ticks(self, ticks_from: int, ticks_to: int) -> RecallScope:
        """orr_scope_create_ticks: the live rows with ticks_from <= CreatedAtUtc.Ticks < ticks_to."""
        h = C.c_void_p()
        N.check(N.hip.orr_scope_create_ticks(self._h, int(ticks_from), int(ticks_to), C.byref(h)))
        return RecallScope(h, self)

    def scope_terms(self, terms: Sequence[bytes], mode: str = "all") -> RecallScope:
        """orr_scope_create_terms: the live rows whose lowercased content contains every term (mode "all") or at least one
        (mode "any") as a substring.  terms: lowercased bytes without whitespace; no terms give an empty scope."""
        modes = {"all": N.ORR_TERMS_ALL, "any": N.ORR_TERMS_ANY}
        if mode not in modes:
            raise ValueError('mode: "all" or "any"')
        pool, toff, _ = pack_terms([list(terms)])
        n_terms = int(toff.shape[0]) - 1
        h = C.c_void_p()
        N.check(N.hip.orr_scope_create_terms(self._h, n_terms, _ptr(pool), _ptr(toff), modes[mode], C.byref(h)))
        return RecallScope(h, self)

    def scope_near(self, probes, min_cosine: float, mode: str = "all") -> RecallScope:
        """orr_scope_create_near: the live rows whose reference cosine to every probe (mode "all") or to at least one
        (mode "any") is >= min_cosine.  probes: [n_probes, dim] float32, numpy or a torch tensor on the device, at most 8;
        no probes give an empty scope; a dim other than the index's gives cosine 0 for every row."""
        n, dim, p, m = _near_args(probes, mode, True)
        h = C.c_void_p()
        N.check(N.hip.orr_scope_create_near(self._h, n, dim, _ptr(p) if n and dim else None, float(min_cosine), m, C.byref(h)))
        return RecallScope(h, self)

    def range_cosine(self, qvecs, min_cosine, max_hits: int, within: Optional[RecallScope] = None):
        """orr_search_range_cosine: for each query EVERY live row (of `within`, when given) whose reference cosine to it is >=
        its own min_cosine[b], with that cosine.  qvecs: [B, dim] float32, numpy or a torch tensor on the device, at most 64;
        min_cosine: B thresholds.  Returns (row_ids, order_keys, cosines, totals): per-query arrays of the best max_hits hits,
        cosine descending then candidate position, and totals [B], the exact number of hits.  OrrError with code ORR_ELIMIT
        (its `totals`: every query's upper bound) when a query is too unselective for "range_pair_cap"."""
        return _range_cosine(N.hip.orr_search_range_cosine, self._h, qvecs, min_cosine, max_hits, within, True)

    def range_cosine_bulk(self, qvecs, min_cosine, max_hits: int, within: Optional[RecallScope] = None):
        """orr_search_range_cosine_bulk: range_cosine for up to 1024 queries in one call -- the same answers as range_cosine on
        slices of 64; from 65 screened queries up (dim % 128 == 0, dim >= 512) the int8 screening GEMM screens them in one
        pass over the shard per launch group.  Takes and returns what range_cosine does."""
        return _range_cosine(N.hip.orr_search_range_cosine_bulk, self._h, qvecs, min_cosine, max_hits, within, True)

    def search_diverse(self, qvecs, queries_terms, now_ticks: int, topk: int, pool: int, mode: str = "collapse", param: float = 0.95,
                       within: Optional[RecallScope] = None, candidate_limit: int = 300):
        """orr_search_batch_diverse: the plain search's best `pool` rows of every query (inside `within`, when given), compared
        with each other by the reference's cosine of the stored rows, and a greedy pass over them in rank order that keeps up
        to topk: mode "collapse" drops a row whose cosine to a kept one is >= param (max_cosine), mode "mmr" picks by
        param * score - (1 - param) * (greatest cosine to a kept row) (param = lambda in [0, 1]).  pool is at most 56; nothing
        outside the pool is looked at, so counts may stay below topk.
        Returns (rows [B,k] int64, fused scores [B,k] float64, counts [B] int32, pool_rank [B,k] int32) in pick order."""
        modes = {"collapse": 0, "mmr": 1}
        if mode not in modes:
            raise ValueError("mode must be 'collapse' or 'mmr'")
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        tpool, toff, qoff = pack_terms(queries_terms)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        ranks = np.full((B, k), -1, dtype=np.int32)
        N.check(N.hip.orr_search_batch_diverse(self._h, B, dim, _ptr(q), _ptr(tpool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                               int(candidate_limit), within._h if within is not None else None, int(pool), modes[mode],
                                               float(param), _ptr(rows), _ptr(scores), _ptr(counts), _ptr(ranks)))
        return rows, scores, counts, ranks

    def keys(self, row_ids, keys) -> RecallKeys:
        """orr_keys_create: a key column over this shard, every row at KEY_NONE, then RecallKeys.set(row_ids, keys)."""
        ids, ks, n = RecallKeys._pairs(row_ids, keys)
        h = C.c_void_p()
        N.check(N.hip.orr_keys_create(self._h, n, _ptr(ids) if n else None, _ptr(ks) if n else None, C.byref(h)))
        return RecallKeys(h, self)

    def scope_keys(self, keys_handle: RecallKeys, keys) -> RecallScope:
        """orr_scope_create_keys: the live rows whose key is one of `keys` (host int64, at most 65,536; duplicates count once;
        KEY_NONE selects the rows without a key; no keys give an empty scope): "search inside these documents"."""
        ks = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        n = int(ks.shape[0])
        h = C.c_void_p()
        N.check(N.hip.orr_scope_create_keys(self._h, keys_handle._h, n, _ptr(ks) if n else None, C.byref(h)))
        return RecallScope(h, self)

    def search_per_key(self, qvecs, queries_terms, now_ticks: int, topk: int, keys: RecallKeys, max_per_key: int = 1, pool: int = 24,
                       within: Optional[RecallScope] = None, candidate_limit: int = 300):
        """orr_search_batch_per_key: the plain search's ranking of every query (inside `within`, when given) walked from the
        top, keeping at most max_per_key rows of each key and every row without one, until topk are kept.  Exact beyond the
        pool: counts stay below topk only when the candidates ran out.  max(1, topk) <= pool <= 56.
        Returns (rows [B,k] int64, fused scores [B,k] float64, keys [B,k] int64, counts [B] int32, rounds [B] int32)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        tpool, toff, qoff = pack_terms(queries_terms)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        rkeys = np.full((B, k), N.ORR_KEY_NONE, dtype=np.int64)
        counts = np.zeros(B, dtype=np.int32)
        rounds = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_search_batch_per_key(self._h, B, dim, _ptr(q), _ptr(tpool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                               int(candidate_limit), within._h if within is not None else None, keys._h,
                                               int(max_per_key), int(pool), _ptr(rows), _ptr(scores), _ptr(rkeys), _ptr(counts),
                                               _ptr(rounds)))
        return rows, scores, rkeys, counts, rounds

    def search_routed(self, docs: "RecallIndex", keys: RecallKeys, qvecs, queries_terms, now_ticks: int, topk: int, route: int,
                      within: Optional[RecallScope] = None, candidate_limit: int = 300):
        """orr_search_batch_routed: per query the best `route` (1 .. 1024) rows of `docs` (a sealed index whose row ids are keys
        of `keys`, normally keys.centroid_index()), then the search inside the rows of this index that carry one of those keys
        (and lie in `within`, when given).  Bit for bit what docs.search, scope_keys(.and_(within)) and search_in_scope give per
        query.  Returns (rows [B,k] int64, fused scores [B,k] float64, counts [B] int32, route_keys [B,route] int64 -- KEY_NONE
        behind the routed ones --, route_n [B] int32)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        tpool, toff, qoff = pack_terms(queries_terms)
        k, r = max(1, int(topk)), max(1, int(route))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        route_keys = np.full((B, r), N.ORR_KEY_NONE, dtype=np.int64)
        route_n = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_search_batch_routed(docs._h, self._h, keys._h, B, dim, _ptr(q), _ptr(tpool), _ptr(toff), _ptr(qoff), now_ticks,
                                              int(route), int(topk), int(candidate_limit), within._h if within is not None else None,
                                              _ptr(rows), _ptr(scores), _ptr(counts), _ptr(route_keys), _ptr(route_n)))
        return rows, scores, counts, route_keys, route_n

    def search_in_scope(self, qvecs, queries_terms, now_ticks: int, topk: int, scope: RecallScope, candidate_limit: int = 300):
        """orr_search_batch_in_scope: search_masked with the scope taken from a handle -- nothing is resolved per call.
        Returns (rows [B,k] int64, scores [B,k] float64, counts [B] int32)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_search_batch_in_scope(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                                int(candidate_limit), scope._h, _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def search_in_scopes(self, qvecs, queries_terms, now_ticks: int, topk: int, scopes: Sequence[RecallScope], query_scope,
                         candidate_limit: int = 300):
        """orr_search_batch_in_scopes: query b searches inside scopes[query_scope[b]]; the large scopes share ONE screening
        pass over the shard.  At most 64 scopes.  Returns (rows [B,k] int64, scores [B,k] float64, counts [B] int32)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        qs = np.ascontiguousarray(query_scope, dtype=np.int32).reshape(-1)
        if qs.shape[0] != B:
            raise ValueError(f"query_scope: {qs.shape[0]} entries for {B} queries")
        handles = (C.c_void_p * max(1, len(scopes)))(*[sc._h for sc in scopes])
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_search_batch_in_scopes(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                                 int(candidate_limit), len(scopes), C.cast(handles, C.c_void_p), _ptr(qs),
                                                 _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def search_shard_scoped(self, qvecs, queries_terms, now_ticks: int, kprime: int, candidate_limit: int, scope_ids,
                            scope_before=None, topk: int = 0, out=None):
        """orr_search_shard_scoped: this shard's [B, kprime+1] records of a scoped search (for merge_candidates).  scope_before
        [B]: each query's scoped live rows on the shards in front (scope_count there), or None."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        n_ids, ids, off = self._scope_args(scope_ids, B)
        before = None if scope_before is None else np.ascontiguousarray(scope_before, dtype=np.int64).reshape(B)
        if out is None:
            out = np.zeros((B, kprime + 1), dtype=CAND_DTYPE)
        N.check(N.hip.orr_search_shard_scoped(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(kprime),
                                              int(candidate_limit), max(0, int(topk)), n_ids, _ptr(ids) if n_ids else None, _ptr(off),
                                              _ptr(before), _ptr(out)))
        return out

    def search_shard_masked(self, qvecs, queries_terms, now_ticks: int, kprime: int, candidate_limit: int, scope_ids,
                            scope_before: int = 0, topk: int = 0, shard_pass: int = 0, out=None):
        """orr_search_shard_masked: this shard's [B, kprime+1] records of a masked search (for merge_candidates).  scope_ids:
        ONE flat list shared by the batch (numpy or torch, host or device); scope_before: the scope's live rows on the shards
        in front (scope_count there); shard_pass: 0 the library's choice (the masked screen where it pays), 1 the list path."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        ids = scope_ids if _is_torch(scope_ids) else np.ascontiguousarray(scope_ids, dtype=np.int64).reshape(-1)
        n_ids = int(ids.shape[0])
        if out is None:
            out = np.zeros((B, kprime + 1), dtype=CAND_DTYPE)
        N.check(N.hip.orr_search_shard_masked(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(kprime),
                                              int(candidate_limit), max(0, int(topk)), int(shard_pass), n_ids, _ptr(ids) if n_ids else None,
                                              int(scope_before), _ptr(out)))
        return out

    def search_shard_in_scope(self, qvecs, queries_terms, now_ticks: int, kprime: int, candidate_limit: int, scope: RecallScope,
                              scope_before: int = 0, topk: int = 0, shard_pass: int = 0, out=None):
        """orr_search_shard_in_scope: search_shard_masked with the scope taken from a handle of this shard (a RecallScope, or
        RecallClusterScope.shard(i)); scope_before: the scope's live rows on the shards in front (their handles' rows)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        if out is None:
            out = np.zeros((B, kprime + 1), dtype=CAND_DTYPE)
        N.check(N.hip.orr_search_shard_in_scope(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(kprime),
                                                int(candidate_limit), max(0, int(topk)), int(shard_pass), scope._h,
                                                int(scope_before), _ptr(out)))
        return out

    def search_shard_in_scopes(self, qvecs, queries_terms, now_ticks: int, kprime: int, candidate_limit: int,
                               scopes: Sequence[RecallScope], query_scope, scope_before, topk: int = 0, shard_pass: int = 0, out=None):
        """orr_search_shard_in_scopes: this shard's [B, kprime+1] records of a grouped search, query b inside
        scopes[query_scope[b]] (handles of this shard: RecallScope, or RecallClusterScope.shard(i)); scope_before [len(scopes)]:
        each scope's live rows on the shards in front (their handles' rows)."""
        B = len(queries_terms)
        dim, q, _keep = self._query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        qs = np.ascontiguousarray(query_scope, dtype=np.int32).reshape(-1)
        if qs.shape[0] != B:
            raise ValueError(f"query_scope: {qs.shape[0]} entries for {B} queries")
        before = np.ascontiguousarray(scope_before, dtype=np.int64).reshape(-1)
        if before.shape[0] != len(scopes):
            raise ValueError(f"scope_before: {before.shape[0]} entries for {len(scopes)} scopes")
        handles = (C.c_void_p * max(1, len(scopes)))(*[sc._h for sc in scopes])
        if out is None:
            out = np.zeros((B, kprime + 1), dtype=CAND_DTYPE)
        N.check(N.hip.orr_search_shard_in_scopes(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(kprime),
                                                 int(candidate_limit), max(0, int(topk)), int(shard_pass), len(scopes),
                                                 C.cast(handles, C.c_void_p), _ptr(qs), _ptr(before), _ptr(out)))
        return out

    def scope_count(self, scope_ids, n_queries: int = 1) -> np.ndarray:
        """orr_index_scope_count: [n_queries] int64, the live rows each query's scope resolves to on this shard."""
        n_ids, ids, off = self._scope_args(scope_ids, n_queries)
        live = np.zeros(n_queries, dtype=np.int64)
        N.check(N.hip.orr_index_scope_count(self._h, int(n_queries), n_ids, _ptr(ids) if n_ids else None, _ptr(off), _ptr(live)))
        return live

    def view(self) -> "RecallIndex":
        """orr_index_view: a second search lane over this sealed shard (own streams and workspaces, shared
        corpus).  Searches on the index and on its views may run concurrently from different threads."""
        h = C.c_void_p()
        N.check(N.hip.orr_index_view(self._h, C.byref(h)))
        v = RecallIndex.__new__(RecallIndex)
        v.__dict__.update(self.__dict__)
        v._h = h
        v._parent = self                     # keeps the owner alive; close views before it
        return v

    def set_option(self, name: str, value: int) -> None:
        N.check(N.hip.orr_index_set_option(self._h, name.encode(), int(value)))

    def screen_dots(self, qvecs) -> np.ndarray:
        """orr_index_screen_dots: the two-stage pass's plain-bf16 screening dots, [B, rows] fp32 (diagnostic)."""
        q = np.ascontiguousarray(qvecs, dtype=np.float32)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        out = np.empty((q.shape[0], self.rows), dtype=np.float32)
        N.check(N.hip.orr_index_screen_dots(self._h, int(q.shape[0]), int(q.shape[1]), _ptr(q), _ptr(out)))
        return out

    def screen_i8_dots(self, qvecs, form: int, nt_rows: bool = False, images: bool = True):
        """orr_index_screen_i8_dots: raw int32 accumulators [B, rows] of one form of the int8 screening GEMM (0 eight-wave,
        1 four-wave 32x32x32, 2 four-wave 16x16x64) and, with images, the int8 images it multiplied ([B, dim], [rows, dim])."""
        q = np.ascontiguousarray(qvecs, dtype=np.float32)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        B, dim, n = int(q.shape[0]), int(q.shape[1]), self.rows
        dots = np.empty((B, n), dtype=np.int32)
        iq = np.empty((B, dim), dtype=np.int8) if images else None
        ie = np.empty((n, dim), dtype=np.int8) if images else None
        N.check(N.hip.orr_index_screen_i8_dots(self._h, B, dim, _ptr(q), int(form), 1 if nt_rows else 0, _ptr(dots), _ptr(iq), _ptr(ie)))
        return dots, iq, ie

    def screen_i8_consts(self, qvecs=None) -> dict:
        """orr_index_screen_i8_consts: the int8 shadow's row constants (scale, rel_err, rel_hat [rows]; rowf [rows, 4]) and, with
        queries, their quantisation's (s1 [B] fp32; err2, err2_level1 [B] fp64; iq2 [B, dim], the second int8 level)."""
        n = self.rows
        out = {"scale": np.empty(n, np.float32), "rel_err": np.empty(n, np.float32), "rel_hat": np.empty(n, np.float32),
               "rowf": np.empty((n, 4), np.float32)}
        B, dim, q = 0, self.dim, None
        if qvecs is not None:
            q = np.ascontiguousarray(qvecs, dtype=np.float32)
            q = q.reshape(1, -1) if q.ndim == 1 else q
            B, dim = int(q.shape[0]), int(q.shape[1])
            out.update(s1=np.empty(B, np.float32), err2=np.empty(B, np.float64), err2_level1=np.empty(B, np.float64),
                       iq2=np.empty((B, dim), np.int8))
        N.check(N.hip.orr_index_screen_i8_consts(self._h, B, dim, _ptr(q), _ptr(out["scale"]), _ptr(out["rel_err"]), _ptr(out["rel_hat"]),
                                                 _ptr(out["rowf"]), _ptr(out.get("s1")), _ptr(out.get("err2")),
                                                 _ptr(out.get("err2_level1")), _ptr(out.get("iq2"))))
        return out

    def screen_i8_stream_dots(self, qvecs, unit16: bool = False) -> np.ndarray:
        """orr_index_screen_i8_stream_dots: raw int32 accumulators [B, 2, rows] (I1, I2) of the streaming int8 screen for 1..4
        queries, in its 128-row-unit form or (unit16, dim % 1024 == 0) its 16-row-unit form."""
        q = np.ascontiguousarray(qvecs, dtype=np.float32)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        out = np.empty((q.shape[0], 2, self.rows), dtype=np.int32)
        N.check(N.hip.orr_index_screen_i8_stream_dots(self._h, int(q.shape[0]), int(q.shape[1]), _ptr(q), 1 if unit16 else 0, _ptr(out)))
        return out

    def pass_dots(self, qvecs, kernel: int) -> np.ndarray:
        """orr_index_pass_dots: fp32 dots [B, rows] of the batched pass's streaming f32 MFMA form (kernel 0) or of the unfused
        split-bf16 GEMM with three products (kernel 1)."""
        q = np.ascontiguousarray(qvecs, dtype=np.float32)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        out = np.empty((q.shape[0], self.rows), dtype=np.float32)
        N.check(N.hip.orr_index_pass_dots(self._h, int(kernel), int(q.shape[0]), int(q.shape[1]), _ptr(q), _ptr(out)))
        return out

    def capture_screen(self, enabled: bool = True) -> None:
        """orr_index_capture_screen: arm the handle -- the first pass through the two-stage screen of the next search records its
        floor and its survivors' buffers (one capture per arming) -- or disarm it."""
        N.check(N.hip.orr_index_capture_screen(self._h, 1 if enabled else 0))

    def captured_screen(self) -> dict:
        """orr_index_captured_screen: the capture the handle holds.  The plan scalars (B, kth, cap, screen, tile_form, scope,
        floor_form, n, prefix_rows, eps3, eps1), floor_key [B] uint64, L [B] float64, cnt [B] uint32 and the buffers key [B, cap]
        uint64 / pos [B, cap] uint32, of which a query's first min(cnt, cap) slots are filled (the rest: key 0, pos 2^32 - 1)."""
        info = N.OrrScreenCapture()
        N.check(N.hip.orr_index_captured_screen(self._h, C.byref(info), 0, 0, None, None, None, None, None))
        B, cap = int(info.B), int(info.cap)
        out = {"floor_key": np.zeros(B, np.uint64), "L": np.zeros(B, np.float64), "cnt": np.zeros(B, np.uint32),
               "key": np.zeros((B, cap), np.uint64), "pos": np.full((B, cap), 0xFFFFFFFF, np.uint32)}
        N.check(N.hip.orr_index_captured_screen(self._h, C.byref(info), B, cap, _ptr(out["floor_key"]), _ptr(out["L"]), _ptr(out["cnt"]),
                                                _ptr(out["key"]), _ptr(out["pos"])))
        out.update({name: getattr(info, name) for name, _ in N.OrrScreenCapture._fields_ if name != "reserved"})
        return out

    def pair_dots(self, lists) -> np.ndarray:
        """orr_index_pair_dots: for every list of up to 56 row positions (candidate order: order_key - row_base) the matrix of the
        exact dots of its rows with each other (the diagonal: a row's exact norm).  Returns [n_lists, stride, stride] float64,
        stride the longest list's length; what lies beyond a list's own length is NaN."""
        lists = [np.ascontiguousarray(l, dtype=np.int64).reshape(-1) for l in lists]
        stride = max([1] + [len(l) for l in lists])
        off = np.zeros(len(lists) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(l) for l in lists])
        pos = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        pos = np.ascontiguousarray(pos if len(pos) else np.zeros(1, np.int64), dtype=np.int64)
        out = np.full((len(lists), stride, stride), np.nan, dtype=np.float64)
        N.check(N.hip.orr_index_pair_dots(self._h, len(lists), _ptr(off), _ptr(pos), stride, _ptr(out)))
        return out

    def keyword_bitmaps(self, terms: Sequence[bytes], form: int = -1, mid: int = -1) -> dict:
        """orr_index_keyword_bitmaps: the keyword chain of a search for one query that owns every term (distinct, none empty, at
        most 4096), seen directly.  form: -1 as a search chooses, 0 all-pairs, 1 lookup; mid: -1 default, 0 tokens of 17..32
        bytes through the wave scan.  Returns bitmaps [n_terms, words] uint32 (raw: deleted positions are not cleared), alias
        [n_terms] uint8, hits, runs (how often the chain ran) and form (the short-token form that ran: 0 all-pairs, 1 lookup)."""
        pool, toff, _ = pack_terms([list(terms)])
        n_terms = int(toff.shape[0]) - 1
        words = ((self.rows + 31) // 32 + 3) // 4 * 4
        bitmaps = np.zeros((max(n_terms, 0), words), dtype=np.uint32)
        alias = np.zeros(max(n_terms, 0), dtype=np.uint8)
        info = np.zeros(4, dtype=np.int64)
        N.check(N.hip.orr_index_keyword_bitmaps(self._h, n_terms, _ptr(pool), _ptr(toff), int(form), int(mid), words,
                                                bitmaps.ctypes.data, alias.ctypes.data, _ptr(info)))
        return {"bitmaps": bitmaps, "alias": alias, "words": int(info[0]), "hits": int(info[1]), "runs": int(info[2]), "form": int(info[3])}

    def set_profiling(self, on) -> None:
        """False/0 off, True/1 every kernel, 2 only the launch that streams every row (orr_index_set_profiling)."""
        N.check(N.hip.orr_index_set_profiling(self._h, int(on)))

    def search_stats(self, reset: bool = False) -> dict:
        """orr_index_search_stats: repeats of the cheap passes and what the screening pass kept, since the last reset."""
        st = N.OrrSearchStats()
        N.check(N.hip.orr_index_search_stats(self._h, C.byref(st), 1 if reset else 0))
        d = {n: int(getattr(st, n)) for n, _ in N.OrrSearchStats._fields_ if n != "reserved"}
        d["survivors_per_query"] = d["survivors_total"] / d["survivor_samples"] if d["survivor_samples"] else None
        return d

    def reset_search_stats(self) -> None:
        N.check(N.hip.orr_index_search_stats(self._h, None, 1))

    def kernel_stats(self) -> dict:
        """orr_index_kernel_stats: every timed name since profiling was switched on (kernels, and host phases such as
        "scope_id_table" or "grouped_screen_pairs").  The call reports how many names there are; the array grows to hold them
        all (a grouped search with a list group beside it uses more than 32)."""
        cap = 64
        while True:
            arr = (N.OrrKernelStat * cap)()
            n = N.hip.orr_index_kernel_stats(self._h, C.cast(arr, C.c_void_p), cap)
            if n <= cap:
                break
            cap = n
        return {arr[i].name.decode(): {"launches": int(arr[i].launches), "total_ms": float(arr[i].total_ms),
                                       "algo_bytes": float(arr[i].algo_bytes)} for i in range(max(n, 0))}


class _BorrowedIndex(RecallIndex):
    """A shard owned by a RecallCluster: usable like a RecallIndex, never destroyed through this object."""

    def __init__(self, handle, dim: int, owner):
        self._h = handle
        self.dim = dim
        self.row_base = 0
        self._owner = owner                  # keeps the cluster alive

    def close(self) -> None:
        self._h = None


class RecallCluster:
    """orr_cluster: several shards (one per entry of `devices`) behind one handle in this process; searches answer as
    one index over all the rows would.  shard(i) is a borrowed RecallIndex to append to (rows of shard i newer than or
    as new as those of shard i + 1; pass explicit row_ids)."""

    def __init__(self, devices: Sequence[int], dim: int, capacity_rows_per_shard: int = 0):
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        N.check(N.hip.orr_cluster_create(_ptr(devs), int(devs.shape[0]), dim, int(capacity_rows_per_shard), C.byref(h)))
        self._h = h
        self.dim = dim

    def close(self) -> None:
        if getattr(self, "_h", None):
            N.hip.orr_cluster_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_shards(self) -> int:
        return int(N.hip.orr_cluster_shards(self._h))

    @property
    def rows(self) -> int:
        return int(N.hip.orr_cluster_rows(self._h))

    def shard(self, i: int) -> RecallIndex:
        p = N.hip.orr_cluster_shard(self._h, int(i))
        if not p:
            N.check(N.ORR_EINVAL)
        return _BorrowedIndex(C.c_void_p(p), self.dim, self)

    def seal(self) -> None:
        N.check(N.hip.orr_cluster_seal(self._h))

    def search(self, qvecs, queries_terms, now_ticks: int, topk: int, candidate_limit: int = 300):
        """orr_cluster_search_batch; qvecs in host memory (numpy) or None."""
        B = len(queries_terms)
        if qvecs is None:
            dim, q = 0, None
        else:
            q = np.ascontiguousarray(qvecs, dtype=np.float32).reshape(B, -1)
            dim = int(q.shape[1])
            q = q if dim > 0 else None
        pool, toff, qoff = pack_terms(queries_terms)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_cluster_search_batch(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                               int(candidate_limit), _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def _host_query_args(self, qvecs, B: int):
        if qvecs is None:
            return 0, None
        q = np.ascontiguousarray(qvecs, dtype=np.float32).reshape(B, -1)
        dim = int(q.shape[1])
        return dim, (q if dim > 0 else None)

    def search_scoped(self, qvecs, queries_terms, now_ticks: int, topk: int, scope_ids, candidate_limit: int = 300, scope_off=None):
        """orr_cluster_search_batch_scoped: RecallIndex.search_scoped over all shards, as one index holding all the rows would
        answer.  qvecs and the scope in host memory (numpy): one flat list shared by all queries, a sequence of per-query lists,
        or -- with scope_off [B+1] given -- the flat list the offsets cut."""
        B = len(queries_terms)
        dim, q = self._host_query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        if scope_off is None:
            n_ids, ids, off = RecallIndex._scope_args(scope_ids, B)
        else:
            ids = np.ascontiguousarray(scope_ids, dtype=np.int64).reshape(-1)
            n_ids, off = int(ids.shape[0]), np.ascontiguousarray(scope_off, dtype=np.uint64)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_cluster_search_batch_scoped(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                                      int(candidate_limit), n_ids, _ptr(ids) if n_ids else None, _ptr(off),
                                                      _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def search_masked(self, qvecs, queries_terms, now_ticks: int, topk: int, scope_ids, candidate_limit: int = 300):
        """orr_cluster_search_batch_masked: RecallIndex.search_masked over all shards -- ONE scope shared by the batch (a flat
        numpy list in host memory), every shard's masked screen at once.  qvecs in host memory (numpy) or None."""
        B = len(queries_terms)
        dim, q = self._host_query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        ids = np.ascontiguousarray(scope_ids, dtype=np.int64).reshape(-1)
        n_ids = int(ids.shape[0])
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_cluster_search_batch_masked(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                                      int(candidate_limit), n_ids, _ptr(ids) if n_ids else None,
                                                      _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def scope(self, row_ids) -> RecallClusterScope:
        """orr_cluster_scope_create: the live rows that carry these ids (numpy, host memory), resolved once on every shard."""
        ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        n_ids = int(ids.shape[0])
        h = C.c_void_p()
        N.check(N.hip.orr_cluster_scope_create(self._h, n_ids, _ptr(ids) if n_ids else None, C.byref(h)))
        return RecallClusterScope(h, self)

    def scope_ticks(self, ticks_from: int, ticks_to: int) -> RecallClusterScope:
        """orr_cluster_scope_create_ticks: the live rows with ticks_from <= CreatedAtUtc.Ticks < ticks_to, on every shard."""
        h = C.c_void_p()
        N.check(N.hip.orr_cluster_scope_create_ticks(self._h, int(ticks_from), int(ticks_to), C.byref(h)))
        return RecallClusterScope(h, self)

    def scope_terms(self, terms: Sequence[bytes], mode: str = "all") -> RecallClusterScope:
        """orr_cluster_scope_create_terms: the live rows whose lowercased content contains every term (mode "all") or at
        least one (mode "any"), on every shard.  terms: lowercased bytes without whitespace; no terms give an empty scope."""
        modes = {"all": N.ORR_TERMS_ALL, "any": N.ORR_TERMS_ANY}
        if mode not in modes:
            raise ValueError('mode: "all" or "any"')
        pool, toff, _ = pack_terms([list(terms)])
        n_terms = int(toff.shape[0]) - 1
        h = C.c_void_p()
        N.check(N.hip.orr_cluster_scope_create_terms(self._h, n_terms, _ptr(pool), _ptr(toff), modes[mode], C.byref(h)))
        return RecallClusterScope(h, self)

    def scope_near(self, probes, min_cosine: float, mode: str = "all") -> RecallClusterScope:
        """orr_cluster_scope_create_near: the live rows whose reference cosine to every probe (mode "all") or to at least
        one (mode "any") is >= min_cosine, on every shard.  probes: [n_probes, dim] float32 in host memory, at most 8."""
        n, dim, p, m = _near_args(probes, mode, False)
        h = C.c_void_p()
        N.check(N.hip.orr_cluster_scope_create_near(self._h, n, dim, _ptr(p) if n and dim else None, float(min_cosine), m, C.byref(h)))
        return RecallClusterScope(h, self)

    def range_cosine(self, qvecs, min_cosine, max_hits: int, within: Optional[RecallClusterScope] = None):
        """orr_cluster_search_range_cosine: RecallIndex.range_cosine over every shard, merged -- the answers of one index
        holding all the rows.  qvecs in host memory (numpy)."""
        return _range_cosine(N.hip.orr_cluster_search_range_cosine, self._h, qvecs, min_cosine, max_hits, within, False)

    def range_cosine_bulk(self, qvecs, min_cosine, max_hits: int, within: Optional[RecallClusterScope] = None):
        """orr_cluster_search_range_cosine_bulk: RecallIndex.range_cosine_bulk over every shard, merged as range_cosine merges."""
        return _range_cosine(N.hip.orr_cluster_search_range_cosine_bulk, self._h, qvecs, min_cosine, max_hits, within, False)

    def search_in_scope(self, qvecs, queries_terms, now_ticks: int, topk: int, scope: RecallClusterScope, candidate_limit: int = 300):
        """orr_cluster_search_batch_in_scope: search_masked with the scope taken from a handle -- no id list goes to the
        shards, nothing is counted or resolved per call.  qvecs in host memory (numpy) or None.
        Returns (rows [B,k] int64, scores [B,k] float64, counts [B] int32)."""
        B = len(queries_terms)
        dim, q = self._host_query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_cluster_search_batch_in_scope(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                                        int(candidate_limit), scope._h, _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def search_in_scopes(self, qvecs, queries_terms, now_ticks: int, topk: int, scopes: Sequence[RecallClusterScope], query_scope,
                         candidate_limit: int = 300):
        """orr_cluster_search_batch_in_scopes: query b searches inside scopes[query_scope[b]], each result what search_in_scope
        returns with that scope; every shard streams its shadow once per batch.  At most 64 scopes.  qvecs in host memory
        (numpy) or None.  Returns (rows [B,k] int64, scores [B,k] float64, counts [B] int32)."""
        B = len(queries_terms)
        dim, q = self._host_query_args(qvecs, B)
        pool, toff, qoff = pack_terms(queries_terms)
        qs = np.ascontiguousarray(query_scope, dtype=np.int32).reshape(-1)
        if qs.shape[0] != B:
            raise ValueError(f"query_scope: {qs.shape[0]} entries for {B} queries")
        handles = (C.c_void_p * max(1, len(scopes)))(*[sc._h for sc in scopes])
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_cluster_search_batch_in_scopes(self._h, B, dim, _ptr(q), _ptr(pool), _ptr(toff), _ptr(qoff), now_ticks,
                                                         int(topk), int(candidate_limit), len(scopes), C.cast(handles, C.c_void_p),
                                                         _ptr(qs), _ptr(rows), _ptr(scores), _ptr(counts)))
        return rows, scores, counts

    def search_diverse(self, qvecs, queries_terms, now_ticks: int, topk: int, pool: int, mode: str = "collapse", param: float = 0.95,
                       within: Optional[RecallClusterScope] = None, candidate_limit: int = 300):
        """orr_cluster_search_batch_diverse: RecallIndex.search_diverse over all shards, as one index holding all the rows would
        answer -- the pool is search (search_in_scope with `within`) for topk = pool, and the pool's rows that lie on other
        shards than the query's home shard travel there for the pair cosines.  qvecs in host memory (numpy) or None.
        Returns (rows [B,k] int64, fused scores [B,k] float64, counts [B] int32, pool_rank [B,k] int32) in pick order."""
        modes = {"collapse": 0, "mmr": 1}
        if mode not in modes:
            raise ValueError("mode must be 'collapse' or 'mmr'")
        B = len(queries_terms)
        dim, q = self._host_query_args(qvecs, B)
        tpool, toff, qoff = pack_terms(queries_terms)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        counts = np.zeros(B, dtype=np.int32)
        ranks = np.full((B, k), -1, dtype=np.int32)
        N.check(N.hip.orr_cluster_search_batch_diverse(self._h, B, dim, _ptr(q), _ptr(tpool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                                       int(candidate_limit), within._h if within is not None else None, int(pool),
                                                       modes[mode], float(param), _ptr(rows), _ptr(scores), _ptr(counts), _ptr(ranks)))
        return rows, scores, counts, ranks

    def keys(self, row_ids, keys) -> RecallClusterKeys:
        """orr_cluster_keys_create: a key column over every shard, every row at KEY_NONE, then RecallClusterKeys.set(row_ids,
        keys).  numpy, host memory."""
        ids, ks, n = RecallClusterKeys._pairs(row_ids, keys)
        h = C.c_void_p()
        N.check(N.hip.orr_cluster_keys_create(self._h, n, _ptr(ids) if n else None, _ptr(ks) if n else None, C.byref(h)))
        return RecallClusterKeys(h, self)

    def scope_keys(self, keys_handle: RecallClusterKeys, keys) -> RecallClusterScope:
        """orr_cluster_scope_create_keys: the live rows whose key is one of `keys` (host int64, at most 65,536), on every shard:
        an ordinary RecallClusterScope."""
        ks = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        n = int(ks.shape[0])
        h = C.c_void_p()
        N.check(N.hip.orr_cluster_scope_create_keys(self._h, keys_handle._h, n, _ptr(ks) if n else None, C.byref(h)))
        return RecallClusterScope(h, self)

    def search_per_key(self, qvecs, queries_terms, now_ticks: int, topk: int, keys: RecallClusterKeys, max_per_key: int = 1, pool: int = 24,
                       within: Optional[RecallClusterScope] = None, candidate_limit: int = 300):
        """orr_cluster_search_batch_per_key: RecallIndex.search_per_key over all shards, as one index holding all the rows would
        answer -- a key closes cluster-wide, and the call looks outside the pool on every shard.  qvecs in host memory (numpy)
        or None.  Returns (rows [B,k] int64, fused scores [B,k] float64, keys [B,k] int64, counts [B] int32, rounds [B] int32)."""
        B = len(queries_terms)
        dim, q = self._host_query_args(qvecs, B)
        tpool, toff, qoff = pack_terms(queries_terms)
        k = max(1, int(topk))
        rows = np.full((B, k), -1, dtype=np.int64)
        scores = np.zeros((B, k), dtype=np.float64)
        rkeys = np.full((B, k), N.ORR_KEY_NONE, dtype=np.int64)
        counts = np.zeros(B, dtype=np.int32)
        rounds = np.zeros(B, dtype=np.int32)
        N.check(N.hip.orr_cluster_search_batch_per_key(self._h, B, dim, _ptr(q), _ptr(tpool), _ptr(toff), _ptr(qoff), now_ticks, int(topk),
                                                       int(candidate_limit), within._h if within is not None else None, keys._h,
                                                       int(max_per_key), int(pool), _ptr(rows), _ptr(scores), _ptr(rkeys), _ptr(counts),
                                                       _ptr(rounds)))
        return rows, scores, rkeys, counts, rounds

    def pair_dots(self, lists) -> np.ndarray:
        """orr_cluster_pair_dots: RecallIndex.pair_dots over all shards; the lists hold GLOBAL order keys (a shard's row_base +
        position), up to 56 each.  Returns [n_lists, stride, stride] float64, stride the longest list's length; what lies
        beyond a list's own length is NaN."""
        lists = [np.ascontiguousarray(l, dtype=np.int64).reshape(-1) for l in lists]
        stride = max([1] + [len(l) for l in lists])
        off = np.zeros(len(lists) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(l) for l in lists])
        keys = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        keys = np.ascontiguousarray(keys if len(keys) else np.zeros(1, np.int64), dtype=np.int64)
        out = np.full((len(lists), stride, stride), np.nan, dtype=np.float64)
        N.check(N.hip.orr_cluster_pair_dots(self._h, len(lists), _ptr(off), _ptr(keys), stride, _ptr(out)))
        return out

    def set_option(self, name: str, value: int) -> None:
        """orr_cluster_set_option ("exchange": 0 pinned host memory, 1 RCCL all-gather)."""
        N.check(N.hip.orr_cluster_set_option(self._h, name.encode(), int(value)))

    def compact(self) -> int:
        """orr_cluster_compact: every shard without its deleted rows, placed in the global order again."""
        done = C.c_int64(0)
        N.check(N.hip.orr_cluster_compact(self._h, C.cast(C.byref(done), C.c_void_p)))
        return int(done.value)

    def insert_rows(self, shard: int, emb, created_ticks, content_lower, content_off=None, row_ids=None) -> int:
        """orr_cluster_insert_rows: rows into sealed shard `shard` in place (they must keep the shards' order: no newer than
        the shard in front, no older than the shard behind); the shards are then placed in the global order again."""
        n, dim, emb, created_ticks, content_lower, content_off, row_ids = RecallIndex._row_args(emb, created_ticks, content_lower, content_off, row_ids)
        done = C.c_int64(0)
        N.check(N.hip.orr_cluster_insert_rows(self._h, int(shard), n, dim, _ptr(emb), _ptr(created_ticks), _ptr(content_lower),
                                              _ptr(content_off), _ptr(row_ids), C.cast(C.byref(done), C.c_void_p)))
        return int(done.value)

    def search_stats(self, reset: bool = False) -> dict:
        st = N.OrrSearchStats()
        N.check(N.hip.orr_cluster_search_stats(self._h, C.byref(st), 1 if reset else 0))
        d = {n: int(getattr(st, n)) for n, _ in N.OrrSearchStats._fields_ if n != "reserved"}
        d["survivors_per_query"] = d["survivors_total"] / d["survivor_samples"] if d["survivor_samples"] else None
        d["rccl_exchanges"] = int(st.reserved[0])
        return d


def merge_candidates(all_records: np.ndarray, index_dim: int, qvecs, queries_terms, now_ticks: int, topk: int, with_certificates: bool = False):
    """orr_merge_candidates over [n_shards, B, kprime+1] records (host).  Returns
    (rows, scores, counts, uncertified) -- with_certificates: (..., uncertified, certified [B] bool) through
    orr_merge_candidates_ex."""
    assert all_records.dtype == CAND_DTYPE and all_records.ndim == 3
    n_shards, B, kp1 = all_records.shape
    all_records = np.ascontiguousarray(all_records)
    if qvecs is None:
        dim, q = 0, None
    else:
        q = np.ascontiguousarray(qvecs, dtype=np.float32).reshape(B, -1)
        dim = int(q.shape[1])
        q = q if dim > 0 else None
    _, _, qoff = pack_terms(queries_terms)
    k = max(1, int(topk))
    rows = np.full((B, k), -1, dtype=np.int64)
    scores = np.zeros((B, k), dtype=np.float64)
    counts = np.zeros(B, dtype=np.int32)
    unc = C.c_int32(0)
    if with_certificates:
        cert = np.zeros(B, dtype=np.uint8)
        N.check(N.hip.orr_merge_candidates_ex(n_shards, B, kp1 - 1, _ptr(all_records), index_dim, dim, _ptr(q), _ptr(qoff),
                                              now_ticks, int(topk), _ptr(rows), _ptr(scores), _ptr(counts),
                                              C.cast(C.byref(unc), C.c_void_p), _ptr(cert)))
        return rows, scores, counts, int(unc.value), cert.astype(bool)
    N.check(N.hip.orr_merge_candidates(n_shards, B, kp1 - 1, _ptr(all_records), index_dim, dim, _ptr(q), _ptr(qoff),
                                       now_ticks, int(topk), _ptr(rows), _ptr(scores), _ptr(counts),
                                       C.cast(C.byref(unc), C.c_void_p)))
    return rows, scores, counts, int(unc.value)


class MicroBatcher:
    """orrh_batcher: coalesces concurrent single-query searches on one RecallIndex into batched
    orr_search_batch calls (include/omnirecall_host.h).  search() blocks and is thread-safe
    (ctypes releases the GIL during the call)."""

    def __init__(self, index: RecallIndex, max_batch: int = 64, max_wait_us: int = 200):
        self._index = index                    # keep the index alive
        self._h = C.c_void_p(N.host.orrh_batcher_create(index._h, max_batch, max_wait_us))
        if not self._h:
            raise ValueError("orrh_batcher_create failed")

    def search(self, qvec, terms: Sequence[bytes], now_ticks: int, topk: int, candidate_limit: int = 300, with_clock: bool = False):
        """One request.  with_clock: also return the clock its batch was answered at (the latest now_ticks of the batch)."""
        q = None if qvec is None else np.ascontiguousarray(qvec, dtype=np.float32).reshape(-1)
        dim = 0 if q is None else int(q.shape[0])
        pool, toff, _ = pack_terms([terms])
        k = max(1, int(topk))
        rows = np.full(k, -1, dtype=np.int64)
        scores = np.zeros(k, dtype=np.float64)
        cnt, clock = C.c_int32(0), C.c_int64(0)
        st = N.host.orrh_batcher_search_at(self._h, dim, _ptr(q) if dim else None, _ptr(pool), _ptr(toff), len(terms),
                                           now_ticks, int(topk), int(candidate_limit), _ptr(rows), _ptr(scores),
                                           C.cast(C.byref(cnt), C.c_void_p), C.cast(C.byref(clock), C.c_void_p))
        if st != N.ORR_OK:
            raise N.OrrError(st, (N.host.orrh_last_error() or b"").decode("utf-8", "replace"))
        if with_clock:
            return rows[:cnt.value], scores[:cnt.value], int(clock.value)
        return rows[:cnt.value], scores[:cnt.value]

    def stats(self):
        b, r, l = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        N.host.orrh_batcher_stats(self._h, C.cast(C.byref(b), C.c_void_p), C.cast(C.byref(r), C.c_void_p),
                                  C.cast(C.byref(l), C.c_void_p))
        return {"batches": b.value, "requests": r.value, "largest_batch": l.value}

    def close(self):
        if getattr(self, "_h", None):
            N.host.orrh_batcher_destroy(self._h)
            self._h = None
