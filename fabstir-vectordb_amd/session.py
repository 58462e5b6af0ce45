"""VectorDbSession / REST search surface over the GPU hybrid index.

Mirrors the observable behaviour of the reference's two public surfaces for the hot path:
  * Node binding  bindings/node/src/session.rs  (search :203-336, add_vectors :340-432, delete)
  * REST handler  src/api/rest.rs               (search :599-677)
Kept: f64 -> f32 narrowing of inputs (bindings/node/src/utils.rs:6-8), dimension latch and mismatch
errors, first-call initialisation with the first <= 10 vectors (session.rs:365-378), score =
1/(1+distance) computed in f32 (session.rs:291,328; rest.rs:653), default threshold 0.0, results in
ascending distance, `_originalId` round trip, ids shown as `vec_<8 hex of BLAKE3>` when no original id
exists (src/core/types.rs:32-34), metadata filters with 3x oversampling (the filter language in metadata_filter.py;
the oversampled search itself is HybridIndex::search_with_filter of the C++ host mirror), saveToS5 /
loadUserVectors over the chunked on-disk format (chunked.py).  Beyond SURVEY §8's rows and kept only because the
surface tests exercise them: setSchema (metadata_schema.py), deleteByMetadata, updateMetadata.  Not built (out of
scope): the S5 network back end, native metadata types.

`blake3()` below is written from the published BLAKE3 specification (the `blake3` crate is not
available here); it is pinned by the official known-answer vector for the empty input.
"""
import struct

import numpy as np

from .index import HybridIndex
from .metadata_schema import MetadataSchema, SchemaError
from .metadata_filter import FilterError, MetadataFilter

# ---------------------------------------------------------------------------------------------
# BLAKE3 (hash mode, 32-byte output) — VectorId::from_string (src/core/types.rs:19-22)
# ---------------------------------------------------------------------------------------------
_IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
_PERM = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
_CHUNK_START, _CHUNK_END, _PARENT, _ROOT = 1, 2, 4, 8
_M32 = 0xFFFFFFFF


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & _M32


def _g(s, a, b, c, d, mx, my):
    s[a] = (s[a] + s[b] + mx) & _M32
    s[d] = _rotr(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & _M32
    s[b] = _rotr(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b] + my) & _M32
    s[d] = _rotr(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & _M32
    s[b] = _rotr(s[b] ^ s[c], 7)


def _compress(cv, block_words, counter, block_len, flags):
    s = list(cv) + list(_IV[:4]) + [counter & _M32, (counter >> 32) & _M32, block_len, flags]
    m = list(block_words)
    for r in range(7):
        _g(s, 0, 4, 8, 12, m[0], m[1])
        _g(s, 1, 5, 9, 13, m[2], m[3])
        _g(s, 2, 6, 10, 14, m[4], m[5])
        _g(s, 3, 7, 11, 15, m[6], m[7])
        _g(s, 0, 5, 10, 15, m[8], m[9])
        _g(s, 1, 6, 11, 12, m[10], m[11])
        _g(s, 2, 7, 8, 13, m[12], m[13])
        _g(s, 3, 4, 9, 14, m[14], m[15])
        if r < 6:
            m = [m[p] for p in _PERM]
    for i in range(8):
        s[i] ^= s[i + 8]
        s[i + 8] ^= cv[i]
    return s


def _words(block):
    return struct.unpack("<16I", block.ljust(64, b"\0"))


def _chunk_output(chunk, counter):
    """(cv, last block words, last block len, flags-without-ROOT) of one <=1024-byte chunk."""
    cv = _IV
    blocks = [chunk[i:i + 64] for i in range(0, len(chunk), 64)] or [b""]
    for i, blk in enumerate(blocks[:-1]):
        flags = _CHUNK_START if i == 0 else 0
        cv = tuple(_compress(cv, _words(blk), counter, 64, flags)[:8])
    last = blocks[-1]
    flags = (_CHUNK_START if len(blocks) == 1 else 0) | _CHUNK_END
    return cv, _words(last), len(last), flags, counter


def blake3(data: bytes) -> bytes:
    chunks = [data[i:i + 1024] for i in range(0, len(data), 1024)] or [b""]
    if len(chunks) == 1:
        cv, w, blen, flags, ctr = _chunk_output(chunks[0], 0)
        out = _compress(cv, w, ctr, blen, flags | _ROOT)
        return struct.pack("<8I", *out[:8])
    # binary tree over chunk chaining values: left subtrees are the largest power of two
    def subtree_cv(lo, hi):
        if hi - lo == 1:
            cv, w, blen, flags, ctr = _chunk_output(chunks[lo], lo)
            return tuple(_compress(cv, w, ctr, blen, flags)[:8])
        n = hi - lo
        left = 1 << ((n - 1).bit_length() - 1)
        l, r = subtree_cv(lo, lo + left), subtree_cv(lo + left, hi)
        return tuple(_compress(_IV, l + r, 0, 64, _PARENT)[:8])

    n = len(chunks)
    left = 1 << ((n - 1).bit_length() - 1)
    l, r = subtree_cv(0, left), subtree_cv(left, n)
    out = _compress(_IV, l + r, 0, 64, _PARENT | _ROOT)
    return struct.pack("<8I", *out[:8])


class VectorId:
    """32-byte BLAKE3 of the string id (src/core/types.rs:9-43)."""

    def __init__(self, s):
        self.bytes = blake3(s.encode("utf-8"))

    def to_string(self):
        return "vec_" + self.bytes[:4].hex()  # `vec_<8 hex>` (src/core/types.rs:32-34)

    def row_id(self):
        return struct.unpack("<Q", self.bytes[:8])[0]  # u64 row id handed to the engine


def js_array_to_vec_f32(v):
    """bindings/node/src/utils.rs:6-8: `x as f32` per element (round to nearest even)."""
    return np.asarray(v, dtype=np.float64).astype(np.float32)


class SessionError(Exception):
    pass


def _score_f32(d):
    """The session's score of a distance, in f32: 1 / (1 + d) (session.rs:291)."""
    return np.float32(1.0) / (np.float32(1.0) + np.float32(d))


def diverse_options(options, k):
    """The diverse-search options of one request: None when it names none of them, else
    (fetch_k, lam, distinct).  "mmrLambda": float in [0, 1], absent = 1 (no re-ranking: "distinct" alone is the
    de-duplicated search); "fetchK": integer in k..256, absent = min(256, 4 k); "distinct": absent = true."""
    if not any(name in options for name in ("mmrLambda", "fetchK", "distinct")):
        return None
    k = int(k)
    try:
        lam = float(options.get("mmrLambda", 1.0))
        fetch_k = int(options.get("fetchK", min(256, 4 * k)))
    except (TypeError, ValueError) as e:
        raise SessionError(f"Invalid mmrLambda or fetchK: {e}") from e
    if not 0.0 <= lam <= 1.0:  # NaN included
        raise SessionError(f"Invalid mmrLambda: {lam!r} (expected a number in [0, 1])")
    if k < 1 or not k <= fetch_k <= 256:
        raise SessionError(f"Invalid fetchK: {fetch_k} (expected k <= fetchK <= 256, with k = {k} >= 1)")
    return fetch_k, float(np.float32(lam)), bool(options.get("distinct", True))


def grouped_options(options, k):
    """The grouped-search options of one request: None when it has no "groupBy", else
    (path, group_size, fetch_k, missing, fill, distinct).  "groupBy": a dotted path; "groupSize": integer >= 1, absent = 1,
    with k * groupSize <= 4096 (k counts groups); "fetchK": integer in 1..4096, absent = min(4096, 4 k groupSize);
    "groupMissing": "drop" (absent) or "own"; "fill": absent = false; "distinct": absent = true.  The combinations that are
    out of scope are refused here: "mmrLambda", "exact", "threshold", and a filter on the oversampling route."""
    if options.get("groupBy") is None:
        return None
    path = options["groupBy"]
    if not isinstance(path, str) or not path:
        raise SessionError(f'Invalid groupBy: {path!r} (expected a dotted path)')
    for name, why in (("mmrLambda", "a diverse selection picks rows, a grouped one picks groups"),
                      ("exact", "the candidates of a grouped search are those of the ordinary search of fetchK"),
                      ("threshold", "a threshold cuts rows, not groups")):
        if name in options and options[name] not in (None, False):
            raise SessionError(f'"groupBy" cannot be combined with "{name}": {why}')
    if options.get("filter") is not None and options.get("filterMode", "oversample") not in ("pushdown", "resident"):
        raise SessionError(f'a grouped search with a filter needs "filterMode": "pushdown" or "resident", not '
                           f'{options.get("filterMode", "oversample")!r}: "oversample" keeps what is left of 3 k candidates, '
                           'while the groups are taken from the fetchK candidates of a search under the allow-set')
    try:
        k = int(k)
        group_size = int(options.get("groupSize", 1))
        fetch_k = int(options.get("fetchK", min(4096, 4 * k * group_size)))
    except (TypeError, ValueError) as e:
        raise SessionError(f"Invalid groupSize or fetchK: {e}") from e
    if k < 1 or group_size < 1 or k * group_size > 4096:
        raise SessionError(f"Invalid groupSize: {group_size} with k = {k} (expected k >= 1, groupSize >= 1, k * groupSize <= 4096)")
    if not 1 <= fetch_k <= 4096:
        raise SessionError(f"Invalid fetchK: {fetch_k} (expected 1 <= fetchK <= 4096)")
    missing = options.get("groupMissing", "drop")
    if missing not in ("drop", "own"):
        raise SessionError(f'Invalid groupMissing: {missing!r} (expected "drop" or "own")')
    return path, group_size, fetch_k, missing, bool(options.get("fill", False)), bool(options.get("distinct", True))


def radius_of_threshold(threshold):
    """The radius that stands for a score threshold: the largest f32 d >= 0 whose score
    f32(1) / (f32(1) + d) is >= threshold, so that "distance bits <= bits(d)" IS the session's predicate and the device's
    total is exact for it.  f32 add and divide are monotone, so the score never rises with d and a bisection over the
    bit patterns of the non-negative f32 values (0 .. +inf, monotone as integers) finds d.  threshold <= 0: +inf (every
    score is >= 0).  threshold > 1: None — no distance qualifies, d = 0 scores exactly 1.  The threshold is compared as
    search() compares it, as an f32.  NaN: SessionError."""
    t = np.float32(threshold)
    if np.isnan(t):
        raise SessionError("Invalid threshold: NaN")
    if t <= np.float32(0.0):
        return np.float32(np.inf)
    if t > np.float32(1.0):
        return None
    at = lambda bits: np.array(bits, np.uint32).view(np.float32)[()]  # noqa: E731
    lo, hi = 0, 0x7F800000  # score(lo) = 1 >= t; score(+inf) = 0 < t
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if _score_f32(at(mid)) >= t:
            lo = mid
        else:
            hi = mid
    return at(lo)


class VectorDbSession:
    """bindings/node/src/session.rs VectorDBSession — search()/addVectors()/deleteVector() on the GPU index."""

    def __init__(self, ctx, now=0.0, storage=None, session_id="session", **hybrid_config):
        self.ctx = ctx
        self.storage = storage                              # get/put store (chunked.DirStorage / MemoryStorage)
        self.session_id = session_id                        # path prefix of save_to_s5 (:636-642)
        self.index = HybridIndex(ctx, **hybrid_config)   # HybridConfig::default unless overridden
        self.vector_dimension = None                        # latched by the first addVectors (:345-357)
        self.metadata = {}                                  # VectorId string -> metadata (with _originalId)
        self._rows = {}                                     # u64 row id -> VectorId string
        self.now = now
        self.destroyed = False
        self.schema = None                                  # MetadataSchema or None (set_schema)
        self._meta_columns = None                           # MetadataColumns, made by the first "resident" filter
        self._filter_info = None                            # last_filter_info()

    # -- add_vectors: session.rs:340-432 -------------------------------------------------------
    def add_vectors(self, vectors):
        """vectors: iterable of dicts {"id": str, "vector": [float], "metadata": any}."""
        if self.destroyed:
            raise SessionError("Session already destroyed")
        vectors = list(vectors)
        if vectors:
            first_dim = len(vectors[0]["vector"])
            if self.vector_dimension is not None and first_dim != self.vector_dimension:
                raise SessionError(f"Vector dimension mismatch: expected {self.vector_dimension}, got {first_dim}")
            if self.vector_dimension is None:
                self.vector_dimension = first_dim
        if not self.index.is_initialized() and vectors:
            training = np.stack([js_array_to_vec_f32(v["vector"]) for v in vectors[:10]])  # first 10 (:367-371)
            self.index.initialize(training)
        stored = []  # row ids this call stored, for the resident metadata columns
        try:
            for inp in vectors:
                if self.schema is not None:  # :388-392, before anything of this vector is stored
                    try:
                        self.schema.validate(inp.get("metadata", {}))
                    except SchemaError as e:
                        raise SessionError(f"Schema validation failed for vector '{inp['id']}': {e}") from e
                vid = VectorId(inp["id"])
                vec = js_array_to_vec_f32(inp["vector"])
                if vec.size != self.vector_dimension:
                    raise SessionError(f"Vector dimension mismatch: expected {self.vector_dimension}, got {vec.size}")
                try:
                    self.index.insert(vid.row_id(), vec, now=self.now)
                except Exception as e:  # index errors surface as strings (bindings/node/src/error.rs:61-65)
                    raise SessionError(f"Failed to add vector: {e}") from e
                md = inp.get("metadata", {})
                if isinstance(md, dict):
                    md = dict(md)
                    md["_originalId"] = inp["id"]
                else:
                    md = {"_originalId": inp["id"], "_userMetadata": md}
                self.metadata[vid.to_string()] = md
                self._rows[vid.row_id()] = vid.to_string()
                stored.append(vid.row_id())
        finally:  # whatever was stored before a failure is in the map, so it is in the columns too
            self._columns_in_step(lambda cols: cols.sync_rows(stored, self._rows, self.metadata) if stored else None)

    addVectors = add_vectors

    # -- search: session.rs:203-336 ------------------------------------------------------------------
    def search(self, query_vector, k, options=None):
        if self.destroyed:
            raise SessionError("Session already destroyed")
        options = options or {}
        q = js_array_to_vec_f32(query_vector)
        if self.vector_dimension is not None and q.size != self.vector_dimension:
            raise SessionError(
                f"Query vector dimension mismatch: expected {self.vector_dimension} dimensions, got {q.size}")
        grouped = grouped_options(options, k)
        if grouped is not None:
            return self._search_grouped([q], k, [options], grouped)[0]
        threshold = np.float32(options.get("threshold", 0.0))
        diverse = diverse_options(options, k)
        if diverse is not None:
            return self._search_diverse([q], k, [options], diverse)[0]
        # "exact" (not in the reference): the k nearest resident rows exactly — HybridIndex.search_exact, or its wide form
        # above 256 — in place of the graph walk and the n_probe nearest lists
        if options.get("exact"):
            if options.get("filter") is not None:
                raise SessionError('"exact" and "filter" cannot be combined: an exact filtered search is not available')
            try:
                exact = self.index.search_exact if int(k) <= 256 else self.index.search_exact_wide
                res = exact(q.reshape(1, -1), int(k), now=self.now)
            except Exception as e:
                raise SessionError(f"Search failed: {e}") from e
            return self._results_of(res[0], threshold, bool(options.get("includeVectors", False)))
        flt = None
        if options.get("filter") is not None:  # session.rs:233-247
            try:
                flt = MetadataFilter.from_json(options["filter"])
            except FilterError as e:
                raise SessionError(f"Invalid filter: {e}") from e
        # "filterMode" (not in the reference): absent or "oversample" = the reference's filter path below; "pushdown" = the
        # filter is evaluated over the metadata map once and the matching ids go down as an allow-set that the device
        # applies inside the search (HybridIndex::search_allowed), so up to k matches come back however selective it is
        # "resident" = "pushdown" with the allow-set evaluated on the device over metadata columns kept in HBM
        # (metadata_columns.py): the same ids in the same order, without the walk over the map
        mode = options.get("filterMode", "oversample")
        if mode not in ("oversample", "pushdown", "resident"):
            raise SessionError(f'Invalid filterMode: {mode!r} (expected "oversample", "pushdown" or "resident")')
        # with a filter: 3 k candidates, keep those whose metadata match, truncate — HybridIndex::search_with_filter of
        # the host mirror (src/hybrid/core.rs:513-549); this side only answers "does this id's metadata match"
        matches = None
        if flt is not None:
            def matches(rid):
                key = self._rows.get(rid)
                return key in self.metadata and flt.matches(self.metadata[key])
        try:
            if flt is not None and mode == "resident":
                allowed = self._resident_allowed(flt)
                res = self.index.search_allowed(q.reshape(1, -1), int(k), allowed, now=self.now)  # defaults: ef 50, nprobe 10
            elif flt is not None and mode == "pushdown":
                allowed = self._allowed_by(flt, "pushdown")
                res = self.index.search_allowed(q.reshape(1, -1), int(k), allowed, now=self.now)  # defaults: ef 50, nprobe 10
            else:
                res = self.index.search_with_filter(q.reshape(1, -1), int(k), matches, now=self.now)  # defaults: ef 50, nprobe 10
        except Exception as e:
            raise SessionError(f"Search failed: {e}") from e
        return self._results_of(res[0], threshold, bool(options.get("includeVectors", False)))  # session.rs:229-231

    # -- diverse search: "mmrLambda" / "fetchK" / "distinct" (no counterpart in the reference) -----
    def _search_diverse(self, qs, k, options_list, diverse):
        """search() / search_many() with the diverse options, which every request of the batch shares: ONE
        HybridIndex.search_diverse of fetchK candidates per query, grouped by filter as search_many groups, and one
        selection on the device.  Results come in pick order; the threshold is applied to the picks afterwards."""
        import json
        fetch_k, lam, distinct = diverse
        group_of_query, allow_sets, group_of_key = [], [], {}
        for i, options in enumerate(options_list):
            if options.get("exact"):
                raise SessionError('"exact" cannot be combined with "mmrLambda" / "fetchK" / "distinct": the candidates of a '
                                   'diverse search are those of the ordinary search of fetchK')
            key = None
            if options.get("filter") is not None:
                mode = options.get("filterMode", "oversample")
                if mode not in ("pushdown", "resident"):
                    raise SessionError(f'a diverse search with a filter needs "filterMode": "pushdown" or "resident", not '
                                       f'{mode!r}: "oversample" keeps what is left of 3 k candidates, while the selection '
                                       'takes the fetchK candidates of a search under the allow-set')
                key = (mode, json.dumps(options["filter"], sort_keys=True, separators=(",", ":")))
            if key not in group_of_key:
                allowed = None
                if key is not None:
                    try:
                        flt = MetadataFilter.from_json(options["filter"])
                    except FilterError as e:
                        raise SessionError(f"Invalid filter: {e}") from e
                    if key[0] == "resident":
                        allowed = self._resident_allowed(flt)
                    else:
                        allowed = self._allowed_by(flt, "pushdown")
                group_of_key[key] = len(allow_sets)
                allow_sets.append(allowed)
            group_of_query.append(group_of_key[key])
        try:
            if len(allow_sets) == 1:  # one filter, or none, for the whole batch
                res, _ = self.index.search_diverse(np.stack(qs), int(k), fetch_k, lam, distinct, now=self.now,
                                                   allowed=allow_sets[0])  # defaults: ef 50, nprobe 10
            else:
                res, _ = self.index.search_diverse_groups(np.stack(qs), int(k), fetch_k, allow_sets,
                                                          np.asarray(group_of_query, np.uint32), lam, distinct, now=self.now)
        except Exception as e:
            raise SessionError(f"Search failed: {e}") from e
        return [self._results_of(res[i], np.float32(o.get("threshold", 0.0)), bool(o.get("includeVectors", False)))
                for i, o in enumerate(options_list)]

    # -- grouped search: "groupBy" / "groupSize" / "fetchK" / "groupMissing" / "fill"  ------------
    def _allowed_by(self, flt, mode):
        """The allow-set of a filter by the route a request chose: "resident" on the device, "pushdown" over the map."""
        if mode == "resident":
            return self._resident_allowed(flt)
        return np.fromiter((rid for rid, name in self._rows.items() if name in self.metadata and flt.matches(self.metadata[name])),
                           np.uint64)

    def _search_grouped(self, qs, k, options_list, grouped):
        """search() / search_many() with "groupBy", which every request of the batch shares: k counts groups.  The requests
        are served filter by filter, one HybridIndex.search_grouped per distinct (mode, filter) — the search of fetchK
        candidates, their keys looked up in the metadata columns in HBM and the selection all on the device.  With
        "fill", every group that is not complete although the candidate list was cut is searched again, all of them in ONE
        HybridIndex.search_allowed_groups call at k = groupSize, each under {"$and": [the request's filter, {path: key}]}
        evaluated by the route the request chose ("resident" where it chose none); the answer replaces the group's hits
        and the group is then complete in the sense "what search_allowed returns under that filter at the session's
        settings".  The set of groups is never searched again: "groupsComplete" reports it."""
        import json
        from .metadata_columns import MetadataColumns
        path, group_size, fetch_k, missing, fill, distinct = grouped
        k = int(k)
        cols = getattr(self, "_meta_columns", None)
        if cols is None:
            cols = self._meta_columns = MetadataColumns(self.ctx, self._rows, self.metadata)
        batches = {}  # (mode, canonical filter) -> [request indices]
        filters = {}
        for i, options in enumerate(options_list):
            key = None
            if options.get("filter") is not None:
                key = (options["filterMode"], json.dumps(options["filter"], sort_keys=True, separators=(",", ":")))
                if key not in filters:
                    try:
                        filters[key] = MetadataFilter.from_json(options["filter"])
                    except FilterError as e:
                        raise SessionError(f"Invalid filter: {e}") from e
            batches.setdefault(key, []).append(i)
        out = [None] * len(qs)
        refill = []  # (request, group position, filter key, key value)
        try:
            for key, members in batches.items():
                allowed = None if key is None else self._allowed_by(filters[key], key[0])
                res = self.index.search_grouped(np.stack([qs[i] for i in members]), k, group_size, fetch_k, cols, path,
                                                distinct=distinct, missing=missing, now=self.now, allowed=allowed,
                                                metadata=self.metadata)
                for b, i in enumerate(members):
                    include = bool(options_list[i].get("includeVectors", False))
                    groups = []
                    for g, (tag, word, ids, ds, _, total) in enumerate(res[b]):
                        own = tag == 0  # FVDB_META_MISSING: one candidate without a key, a group of its own
                        entry = {"key": None if own else cols.decode_key(tag, word),
                                 "hits": self._results_of((ids, ds), np.float32(0.0), include), "total": total,
                                 "complete": own or res.group_complete(b, g)}
                        if own:
                            entry["missing"] = True
                        elif fill and not entry["complete"]:
                            refill.append((i, g, key, entry["key"]))
                        groups.append(entry)
                    out[i] = {"groups": groups, "groupsComplete": res.groups_complete(b)}
            if refill:
                from .metadata_filter import MetadataFilter as F
                sets = []
                for i, g, key, value in refill:
                    leaf = F("equals", field=path, value=value)
                    flt = leaf if key is None else F("and", filters=[filters[key], leaf])
                    sets.append(self._allowed_by(flt, "resident" if key is None else key[0]))
                res = self.index.search_allowed_groups(np.stack([qs[i] for i, _, _, _ in refill]), group_size, sets,
                                                       np.arange(len(refill), dtype=np.uint32), now=self.now)
                for j, (i, g, _, _) in enumerate(refill):
                    entry = out[i]["groups"][g]
                    entry["hits"] = self._results_of(res[j], np.float32(0.0), bool(options_list[i].get("includeVectors", False)))
                    entry["complete"] = True
        except SessionError:
            raise
        except Exception as e:
            raise SessionError(f"Search failed: {e}") from e
        return out

    # -- search_within: every row whose score clears a threshold (no counterpart in the reference) -------------------
    def search_within(self, query_vector, threshold, options=None):
        """Every resident row whose score 1/(1+distance) is >= threshold, where search(k, {"threshold": t}) returns at most
        k of them and cannot say how many there are: HybridIndex.search_radius at radius_of_threshold(threshold), at
        search()'s settings (n_probe 10; the recent part exact).  Returns {"results": the entries search() builds, nearest
        first, at most options["maxResults"] (default 4096, 1..4096) of them; "total": how many rows clear the threshold,
        never capped; "truncated": total > len(results)}.  options: "maxResults", "includeVectors", and "filter" with
        "filterMode" "pushdown" (the default here) or "resident" — the matching ids go down as an allow-set as in
        search(), and rows outside it are in neither the results nor the total.  "oversample" keeps what is left of 3 k
        candidates: it has no meaning where nothing is asked for by count, and is refused."""
        if self.destroyed:
            raise SessionError("Session already destroyed")
        options = options or {}
        q = js_array_to_vec_f32(query_vector)
        if self.vector_dimension is not None and q.size != self.vector_dimension:
            raise SessionError(
                f"Query vector dimension mismatch: expected {self.vector_dimension} dimensions, got {q.size}")
        radius = radius_of_threshold(threshold)
        max_results = int(options.get("maxResults", 4096))
        allowed = None
        if options.get("filter") is not None:
            mode = options.get("filterMode", "pushdown")
            if mode not in ("pushdown", "resident"):
                raise SessionError(f'Invalid filterMode for search_within: {mode!r} (expected "pushdown" or "resident"; '
                                   '"oversample" applies to a search by count)')
            try:
                flt = MetadataFilter.from_json(options["filter"])
            except FilterError as e:
                raise SessionError(f"Invalid filter: {e}") from e
            if mode == "resident":
                allowed = self._resident_allowed(flt)
            else:
                allowed = self._allowed_by(flt, "pushdown")
        elif options.get("filterMode") == "oversample":
            raise SessionError('Invalid filterMode for search_within: "oversample" applies to a search by count')
        if radius is None:  # threshold > 1: no score reaches it
            return {"results": [], "total": 0, "truncated": False}
        try:
            res, totals = self.index.search_radius(q.reshape(1, -1), radius, max_results, now=self.now, allowed=allowed)
        except Exception as e:
            raise SessionError(f"Search failed: {e}") from e
        results = self._results_of(res[0], np.float32(threshold), bool(options.get("includeVectors", False)))
        total = int(totals[0])
        return {"results": results, "total": total, "truncated": total > len(results)}

    searchWithin = search_within

    # -- "resident" filters: metadata columns in HBM (metadata_columns.py) -------------------------------------------
    def _resident_allowed(self, flt):
        """The allow-set of `flt` from the metadata columns: the ids "pushdown" computes, in the same order."""
        from .metadata_columns import MetadataColumns
        cols = getattr(self, "_meta_columns", None)
        if cols is None:
            cols = self._meta_columns = MetadataColumns(self.ctx, self._rows, self.metadata)
        allowed, info = cols.evaluate(flt, self.metadata)
        self._filter_info = info
        return allowed

    def _columns_in_step(self, update):
        """update(columns) where a table exists.  The map is the truth: if the table cannot follow it (an engine error, no
        memory), the table is dropped and the next "resident" filter rebuilds it from the map, so the caller's own
        outcome — its result or the error it is raising — stands."""
        cols = getattr(self, "_meta_columns", None)
        if cols is None:
            return
        try:
            update(cols)
        except Exception:  # noqa: BLE001
            self.refresh_metadata_columns()

    def refresh_metadata_columns(self):
        """For callers who changed `session.metadata` directly: the columns are dropped and rebuilt from the map by the
        next "resident" filter."""
        cols = getattr(self, "_meta_columns", None)
        if cols is not None:
            cols.close()
        self._meta_columns = None

    def last_filter_info(self):
        """What the last "resident" filter did: route ("device", or "host" when the filter exceeds the engine's program
        limits and the map was walked), slots, matches, unknown (slots the device left to the host), columns_created,
        and the milliseconds of each step.  None before the first one."""
        info = getattr(self, "_filter_info", None)
        return None if info is None else dict(info)

    def _results_of(self, hits, threshold, include_vectors):
        """One query's (ids, distances) as the result list search() returns: score, threshold, metadata, vectors."""
        out = []
        ids, ds = hits
        pairs = list(zip(ids.tolist(), ds.tolist()))
        kept = []
        for rid, d in pairs:
            score = np.float32(1.0) / (np.float32(1.0) + np.float32(d))
            if not score >= threshold:
                continue
            kept.append((rid, score))
        vectors = {}
        if include_vectors and kept:  # session.rs:266-281: the recent index first, then the historical one; one call
            try:
                rows, found = self.index.get_vectors(np.array([rid for rid, _ in kept], np.uint64))
            except Exception as e:
                raise SessionError(f"Search failed: {e}") from e
            # the f32 values widened to doubles (utils.rs:12-14); an id neither part holds has no vector
            vectors = {rid: [float(v) for v in rows[i]] for i, (rid, _) in enumerate(kept) if found[i]}
        for rid, score in kept:
            key = self._rows.get(rid, f"row_{rid}")
            md = dict(self.metadata.get(key, {}))
            rid_out = key
            if isinstance(md.get("_originalId"), str):
                rid_out = md.pop("_originalId")
                if "_userMetadata" in md:
                    md = md.pop("_userMetadata")
            item = {"id": rid_out, "score": float(score), "metadata": md}
            if include_vectors:
                item["vector"] = vectors.get(rid)
            out.append(item)
        return out

    # -- search_many: a batch of requests, each with its own options (no counterpart in the reference) -----------
    def search_many(self, query_vectors, k, options_list=None):
        """search(query_vectors[i], k, options_list[i]) for every i, served by ONE index call
        (HybridIndex.search_allowed_groups): each distinct filter is evaluated over the metadata map once and becomes one
        allow-set, requests with equal filters (equal canonical JSON) share it, requests without a filter take the
        "no filter" group.  A filtered request must say "filterMode": "pushdown" or "resident" (the allow-set evaluated on
        the device; groups are keyed by mode and filter) — the oversampling path keeps what is left
        of 3 k candidates and cannot share a batch.  Returns one result list per query."""
        import json
        if self.destroyed:
            raise SessionError("Session already destroyed")
        n = len(query_vectors)
        options_list = [{} for _ in range(n)] if options_list is None else [o or {} for o in options_list]
        if len(options_list) != n:
            raise SessionError(f"search_many: {n} queries but {len(options_list)} option sets")
        # "groupBy" (DESIGN.md section 9v): all requests or none, and the same grouping; each request keeps its own filter
        grouped = [grouped_options(o, k) for o in options_list]
        if any(g is not None for g in grouped):
            if any(g != grouped[0] for g in grouped):
                raise SessionError('search_many: "groupBy" and its options must have the same values in every request of a batch')
            qs = []
            for qv in query_vectors:
                q = js_array_to_vec_f32(qv)
                if self.vector_dimension is not None and q.size != self.vector_dimension:
                    raise SessionError(
                        f"Query vector dimension mismatch: expected {self.vector_dimension} dimensions, got {q.size}")
                qs.append(q)
            return self._search_grouped(qs, k, options_list, grouped[0])
        # the diverse options ("mmrLambda", "fetchK", "distinct"): all requests or none, and the same values
        diverse = [diverse_options(o, k) for o in options_list]
        if any(d is not None for d in diverse):
            if any(d != diverse[0] for d in diverse):
                raise SessionError('search_many: "mmrLambda" / "fetchK" / "distinct" must have the same values in every request '
                                   'of a batch (one search of fetchK and one selection serve it)')
            qs = []
            for qv in query_vectors:
                q = js_array_to_vec_f32(qv)
                if self.vector_dimension is not None and q.size != self.vector_dimension:
                    raise SessionError(
                        f"Query vector dimension mismatch: expected {self.vector_dimension} dimensions, got {q.size}")
                qs.append(q)
            return self._search_diverse(qs, k, options_list, diverse[0])
        qs, group_of_query, allow_sets, group_of_key = [], [], [], {}
        for i, (qv, options) in enumerate(zip(query_vectors, options_list)):
            q = js_array_to_vec_f32(qv)
            if self.vector_dimension is not None and q.size != self.vector_dimension:
                raise SessionError(
                    f"Query vector dimension mismatch: expected {self.vector_dimension} dimensions, got {q.size}")
            qs.append(q)
            key = None
            if options.get("filter") is not None:
                mode = options.get("filterMode", "oversample")
                if mode not in ("pushdown", "resident"):
                    raise SessionError(f'search_many: request {i} has a filter with filterMode {mode!r}; a filtered request '
                                       'in a batch needs "filterMode": "pushdown" or "resident"')
                key = (mode, json.dumps(options["filter"], sort_keys=True, separators=(",", ":")))
            if key not in group_of_key:
                allowed = None
                if key is not None:
                    try:
                        flt = MetadataFilter.from_json(options["filter"])
                    except FilterError as e:
                        raise SessionError(f"Invalid filter: {e}") from e
                    if key[0] == "resident":
                        allowed = self._resident_allowed(flt)
                    else:
                        allowed = self._allowed_by(flt, "pushdown")
                group_of_key[key] = len(allow_sets)
                allow_sets.append(allowed)
            group_of_query.append(group_of_key[key])
        if n == 0:
            return []
        try:
            res = self.index.search_allowed_groups(np.stack(qs), int(k), allow_sets, np.asarray(group_of_query, np.uint32),
                                                   now=self.now)  # defaults: ef 50, nprobe 10
        except Exception as e:
            raise SessionError(f"Search failed: {e}") from e
        return [self._results_of(res[i], np.float32(o.get("threshold", 0.0)), bool(o.get("includeVectors", False)))
                for i, o in enumerate(options_list)]

    searchMany = search_many

    def evaluate_search_quality(self, queries, k, options=None):
        """Recall and precision of search() against the exact search over the same resident rows (no counterpart in the
        reference's session): HybridIndex.evaluate_search_quality, or its wide form above k = 256, at search()'s
        settings (ef 50, n_probe 10) unless options "hnswEf" / "ivfNProbe" say otherwise.  Returns avg_recall,
        avg_precision, avg_query_time_ms, queries_evaluated."""
        if self.destroyed:
            raise SessionError("Session already destroyed")
        options = options or {}
        qs = [js_array_to_vec_f32(qv) for qv in queries]
        for q in qs:
            if self.vector_dimension is not None and q.size != self.vector_dimension:
                raise SessionError(
                    f"Query vector dimension mismatch: expected {self.vector_dimension} dimensions, got {q.size}")
        if not qs:
            raise SessionError("Evaluation failed: No test queries provided")
        try:
            fn = self.index.evaluate_search_quality if int(k) <= 256 else self.index.evaluate_search_quality_wide
            return fn(np.stack(qs), int(k), now=self.now, hnsw_ef=int(options.get("hnswEf", 50)),
                      ivf_n_probe=int(options.get("ivfNProbe", 10)))
        except Exception as e:
            raise SessionError(f"Evaluation failed: {e}") from e

    evaluateSearchQuality = evaluate_search_quality

    def quality_grid(self, queries, k, efs, n_probes):
        """evaluate_search_quality at every pair of the listed "hnswEf" and "ivfNProbe" values in one call (no counterpart
        in the reference's session): HybridIndex.quality_grid over the same resident rows, at the session's clock.
        Returns efs, n_probes, avg_recall and avg_precision ([E][P]), avg_query_time_ms, queries_evaluated."""
        if self.destroyed:
            raise SessionError("Session already destroyed")
        qs = [js_array_to_vec_f32(qv) for qv in queries]
        for q in qs:
            if self.vector_dimension is not None and q.size != self.vector_dimension:
                raise SessionError(
                    f"Query vector dimension mismatch: expected {self.vector_dimension} dimensions, got {q.size}")
        if not qs:
            raise SessionError("Evaluation failed: No test queries provided")
        try:
            return self.index.quality_grid(np.stack(qs), int(k), efs, n_probes, now=self.now)
        except Exception as e:
            raise SessionError(f"Evaluation failed: {e}") from e

    qualityGrid = quality_grid

    def delete_vector(self, id):
        vid = VectorId(id)
        if self.destroyed:
            raise SessionError("Session already destroyed")
        try:
            self.index.delete(vid.row_id(), self.now)
        except Exception as e:
            raise SessionError(f"Failed to delete vector: {e}") from e
        self.metadata.pop(vid.to_string(), None)  # :464-467
        self._columns_in_step(lambda cols: cols.set_absent(vid.row_id()))

    deleteVector = delete_vector

    # -- delete_by_metadata: session.rs:489-578 ----------------------------------------------------
    def delete_by_metadata(self, flt):
        """Soft-delete every vector whose metadata matches the simple field filter (`matches_filter` below).
        Returns {"deleted_count", "deleted_ids"} with the user's original ids."""
        if self.destroyed:
            raise SessionError("Session already destroyed")
        matching = []
        for key, md in self.metadata.items():
            if matches_filter(md, flt):
                oid = md.get("_originalId") if isinstance(md, dict) else None
                matching.append((key, oid if isinstance(oid, str) else key))
        ok = 0
        for _, oid in matching:  # batch_delete (src/hybrid/core.rs:968-986): failures are counted, not raised
            try:
                self.index.delete(VectorId(oid).row_id(), self.now)
                ok += 1
            except Exception:  # noqa: BLE001
                pass
        done = matching[:ok]  # the first `successful` entries, as the reference takes them (:553-558)
        for key, _ in done:
            self.metadata.pop(key, None)
        # the entries are gone from the map, so their slots are not present any more
        self._columns_in_step(lambda cols: cols.set_absent_many([VectorId(oid).row_id() for _, oid in done]))
        return {"deleted_count": ok, "deleted_ids": [oid for _, oid in done]}

    deleteByMetadata = delete_by_metadata

    # -- update_metadata: session.rs:581-632 -------------------------------------------------------
    def update_metadata(self, id, metadata):
        if self.destroyed:
            raise SessionError("Session already destroyed")
        key = VectorId(id).to_string()
        if self.schema is not None:  # :592-598
            try:
                self.schema.validate(metadata)
            except SchemaError as e:
                raise SessionError(f"Schema validation failed for vector '{id}': {e}") from e
        if key not in self.metadata:
            raise SessionError(f"Vector with id '{id}' does not exist")
        if isinstance(metadata, dict):
            md = dict(metadata)
            md["_originalId"] = id
        else:
            md = {"_originalId": id, "_userMetadata": metadata}
        self.metadata[key] = md
        def rewrite(cols):
            rid = VectorId(id).row_id()
            if rid in self._rows:
                cols.sync_rows([rid], self._rows, self.metadata)

        self._columns_in_step(rewrite)

    updateMetadata = update_metadata

    def set_schema(self, schema_json):
        """session.rs:742-765: a schema in serde's JSON shape (metadata_schema.py), or None to switch validation off."""
        if self.destroyed:
            raise SessionError("Session already destroyed")
        if schema_json is None:
            self.schema = None
            return
        try:
            self.schema = MetadataSchema.from_json(schema_json)
        except ValueError as e:
            raise SessionError(f"Invalid schema format: {e}") from e

    setSchema = set_schema

    def vacuum(self):
        """session.rs:793-810: physically remove soft-deleted vectors; returns VacuumStats."""
        if self.destroyed:
            raise SessionError("Session already destroyed")
        try:
            return self.index.vacuum()
        except Exception as e:
            raise SessionError(f"Vacuum failed: {e}") from e

    # -- save_to_s5 / load_user_vectors: session.rs:636-697, :99-198 ----------------------------------
    def save_to_s5(self):
        """Chunked index under `session_id/` plus `metadata_map.cbor`; returns the path identifier."""
        from . import chunked
        if self.destroyed:
            raise SessionError("Session already destroyed")
        if self.storage is None:
            raise SessionError("Failed to save to S5: no storage configured")
        ids = {rid: VectorId(md["_originalId"]).bytes for rid, key in self._rows.items()
               for md in [self.metadata.get(key, {})] if isinstance(md.get("_originalId"), str)}
        try:
            chunked.save_index_chunked(self.index, self.storage, self.session_id, id_table=ids, now=self.now)
        except chunked.PersistenceError as e:
            raise SessionError(f"Failed to save index: {e}") from e
        self.storage.put(f"{self.session_id}/metadata_map.cbor", chunked.cbor_encode(self.metadata))
        if self.schema is not None:  # :680-692
            import json
            self.storage.put(f"{self.session_id}/schema.json", json.dumps(self.schema.to_json()).encode())
        return self.session_id

    saveToS5 = save_to_s5

    def load_user_vectors(self, cid, options=None):
        """Replace the index with the one saved under `cid/` (HybridConfig::default, :118) and the metadata map with
        `cid/metadata_map.cbor` (cleared when absent, :139-157)."""
        from . import chunked
        if self.destroyed:
            raise SessionError("Session already destroyed")
        if self.storage is None:
            raise SessionError("Failed to load from S5: no storage configured")
        try:
            index, table = chunked.load_index_chunked(self.ctx, self.storage, cid, now=self.now)
        except chunked.PersistenceError as e:
            if e.kind == "MissingComponent":
                raise SessionError(f"Missing index component: {e}") from e
            if e.kind == "IncompatibleVersion":
                raise SessionError(f"Incompatible index version: {e}") from e
            raise SessionError(f"Failed to load index: {e}") from e
        self.index = index
        self.refresh_metadata_columns()  # another set of rows: the columns are rebuilt by the next "resident" filter
        self._rows = {rid: chunked.display_id(b) for rid, b in table.items()}
        data = self.storage.get(f"{cid}/metadata_map.cbor")
        if data is None:
            self.metadata = {}
        else:
            try:
                md = chunked.cbor_decode(data)
            except ValueError as e:
                raise SessionError(f"Failed to deserialize metadata: {e}") from e
            if not isinstance(md, dict):
                raise SessionError("Failed to deserialize metadata: expected a map")
            self.metadata = chunked.plain(md)
        raw = self.storage.get(f"{cid}/schema.json")  # :159-196: replaced by the saved one, or cleared
        if raw is None:
            self.schema = None
        else:
            import json
            try:
                self.schema = MetadataSchema.from_json(json.loads(raw.decode("utf-8")))
            except (ValueError, UnicodeDecodeError) as e:
                raise SessionError(f"Failed to deserialize schema: {e}") from e

    loadUserVectors = load_user_vectors

    def get_stats(self):
        # session.rs:699-722: vector_count is the ACTIVE count (soft-deleted rows excluded)
        if self.destroyed:
            raise SessionError("Session already destroyed")
        hnsw, ivf = self.index.hnsw(), self.index.ivf()
        hnsw_deleted = hnsw.node_count() - hnsw.active_count()
        ivf_deleted = ivf.total_vectors() - ivf.active_count()
        return {"vector_count": hnsw.active_count() + ivf.active_count(), "index_type": "hybrid",
                "hnsw_vector_count": self.index.recent_count(), "ivf_vector_count": self.index.historical_count(),
                "hnsw_deleted_count": hnsw_deleted, "ivf_deleted_count": ivf_deleted,
                "total_deleted_count": hnsw_deleted + ivf_deleted}

    def graph_health(self, reach=True, components=True):
        """HNSWIndex.graph_health of the recent part (no counterpart in the reference's session)."""
        if self.destroyed:
            raise SessionError("Session already destroyed")
        return self.index.hnsw().graph_health(reach=reach, components=components)

    def destroy(self):
        self.refresh_metadata_columns()
        self.destroyed = True
        self.index = None


def matches_filter(metadata, flt):
    """bindings/node/src/session.rs:831-889: every filter field must be present (dotted paths descend) and equal —
    or, when the metadata value is an array, contain the filter value.  A non-object filter matches nothing, an
    empty one everything."""
    from .metadata_filter import json_eq
    if not isinstance(flt, dict):
        return False
    for key, want in flt.items():
        cur = metadata
        for part in (key.split(".") if "." in key else [key]):
            if isinstance(cur, dict) and part in cur:
                cur = cur[part]
            else:  # Value::get(&str) finds nothing in arrays and scalars
                return False
        if isinstance(cur, list):
            if not any(json_eq(x, want) for x in cur):
                return False
        elif not json_eq(cur, want):
            return False
    return True


def rest_search(index, request, id_of_row=None, now=0.0):
    """POST /api/v1/search (src/api/rest.rs:599-677) for one request dict {"vector": [...], "k": int,
    "options": {...}}.  Like the handler, the hybrid search runs with the default config (the handler builds a
    HybridSearchConfig but calls `hybrid_index.search(&vector, k)`, :631-634)."""
    import time
    vec = np.asarray(request["vector"], dtype=np.float32)
    if vec.size == 0:
        raise ValueError("Vector cannot be empty")  # validate_vector (:741-746) -> 400
    k = int(request["k"])
    opts = request.get("options") or {}
    t0 = time.perf_counter()
    res = index.search(vec.reshape(1, -1), k, now=now)
    ids, ds = res[0]
    results = []
    for rid, d in zip(ids.tolist(), ds.tolist()):
        score = float(np.float32(1.0) / (np.float32(1.0) + np.float32(d)))
        item = {"id": id_of_row(rid) if id_of_row else f"row_{rid}", "distance": float(np.float32(d)), "score": score}
        if opts.get("include_metadata", False):
            item["metadata"] = {}
        results.append(item)
    if opts.get("score_threshold") is not None:
        results = [r for r in results if r["score"] >= opts["score_threshold"]]
    sr, sh = opts.get("search_recent", True), opts.get("search_historical", True)
    return {"results": results, "search_time_ms": (time.perf_counter() - t0) * 1e3,
            "indices_searched": 2 if (sr and sh) else 1, "partial_results": False}


def rest_insert_vector(index, request, now=0.0, rows=None):
    """POST /api/v1/vectors (src/api/rest.rs:392-446) for {"id": str, "vector": [...], "metadata": any}: the vector
    goes in with timestamp = now, so it lands in the recent (HNSW) index.  Returns (201, body); an empty vector raises
    ValueError (400), an index error RuntimeError (500) with the handler's message.  `rows`: dict filled with
    row id -> request id, for rest_search's id_of_row."""
    from .chunked import format_timestamp
    vec = np.asarray(request["vector"], dtype=np.float32)
    if vec.size == 0:
        raise ValueError("Vector cannot be empty")
    vid = VectorId(request["id"])
    try:
        index.insert_with_timestamp(vid.row_id(), vec, now, now)
    except Exception as e:
        raise RuntimeError(f"Failed to add vector to index: {e}") from e
    if rows is not None:
        rows[vid.row_id()] = request["id"]
    # chrono's to_rfc3339() writes UTC as "+00:00" (its serde form, used on disk, writes "Z")
    return 201, {"id": request["id"], "index": "recent", "timestamp": format_timestamp(now)[:-1] + "+00:00"}


def rest_batch_insert(index, request, now=0.0, rows=None):
    """POST /api/v1/vectors/batch (src/api/rest.rs:449-531): per-vector outcome, never an error as a whole."""
    ok, errors = 0, []
    for v in request["vectors"]:
        vec = np.asarray(v["vector"], dtype=np.float32)
        if vec.size == 0:
            errors.append({"id": v["id"], "error": "Vector cannot be empty"})
            continue
        vid = VectorId(v["id"])
        try:
            index.insert_with_timestamp(vid.row_id(), vec, now, now)
        except Exception as e:  # noqa: BLE001
            errors.append({"id": v["id"], "error": f"Index error: {e}"})
            continue
        if rows is not None:
            rows[vid.row_id()] = v["id"]
        ok += 1
    return {"successful": ok, "failed": len(errors), "errors": errors}
