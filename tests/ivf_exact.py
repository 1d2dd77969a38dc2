"""Exact CPU reference of IVF retrieval (mfx_rec_ivf_probe, mfx_rec_query_ivf), made of the references already here: the
probe is the reference top-N of rec_exact.py over the score chains against the centroids, and the query is the candidate
re-ranking of cand_exact.py over the ascending union of the probed lists.

Below the reference: the launch arithmetic of csrc/rec_ivf.hip restated in Python (tile_class ... geometry),
and the cases of tests/test_gpu_ivf_geometry.py (tile_case, boundary_case, long_case, large_case, chunk_case).  The cases
live here so that tests/test_ivf_host.py can assert on the CPU which class of the library's arithmetic each of them lands
in and which property its reference output has; the GPU module then compares the library with that reference."""
import functools
import types

import numpy as np

from cand_exact import exclusion, expected_candidates, regime_factors
from rec_exact import PAD, chain_scores, eligible_mask, expected_topn


def lists_of(assign, nlist):
    """(list_ptr uint32 [nlist + 1], list_idx uint32 [cols]) of an assignment: list l holds its items in ascending id."""
    assign = np.asarray(assign, np.int64)
    ptr = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(assign, minlength=nlist), out=ptr[1:])
    return ptr.astype(np.uint32), np.argsort(assign, kind="stable").astype(np.uint32)


def expected_probe(W, centroids, users, nprobe):
    """(lists uint32 [U, nprobe], scores float32 [U, nprobe]): score descending, then list id ascending; NaN never; padded."""
    return expected_topn(chain_scores(W, centroids, users), True, nprobe)


def union_lists(probes, list_ptr, list_idx):
    """CSR (ptr uint32 [U + 1], idx uint32) of every slot's ascending union of its probed lists (PAD: no list)."""
    list_ptr = np.asarray(list_ptr, np.int64)
    rows = []
    for pr in np.asarray(probes):
        parts = [list_idx[list_ptr[l]:list_ptr[l + 1]] for l in pr if l != PAD]
        rows.append(np.sort(np.concatenate(parts)) if parts else np.zeros(0, np.uint32))
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    idx = np.concatenate(rows) if rows else np.zeros(0, np.uint32)
    return ptr.astype(np.uint32), idx.astype(np.uint32)


def expected_query(S, probes, list_ptr, list_idx, eligible, n_top):
    """(items, scores, n_eligible) of the slots' scores S [U, cols] and their probed lists: expected_candidates over the unions."""
    ptr, idx = union_lists(probes, list_ptr, list_idx)
    return expected_candidates(S, ptr, idx, eligible, n_top)


def pair_counts(probes, list_ptr):
    """int64 [nlist]: the (slot, probe position) pairs of a batch that a work item passes, per list.  A pair without a list
    (PAD) or with an empty list is padding and counts nowhere."""
    sizes = np.diff(np.asarray(list_ptr, np.int64))
    pr = np.asarray(probes).astype(np.int64).ravel()
    pr = pr[pr != PAD]
    return np.bincount(pr[sizes[pr] > 0], minlength=sizes.size)


# ------------------------------------------------------------------------------------------------ the launch arithmetic
USERS_PER_ITEM = 128        # kRecUsers: pairs of one work item, slots of one probe workgroup
TILE = 32                   # kTile: items (or centroids) per tile
SCAN_THREADS = 256          # threads of mfx_ivf_scan
MAX_MERGE = 8192            # kMaxMerge: slices * n_top of one merge
WORKSPACE = 1 << 30         # kWorkspaceCap: bytes of candidate lists per launch
POS_BITS = 10               # kPosBits: a pair is slot << 10 | probe position
CUS = 256                   # compute units of an MI355X (the host test's assumption; the GPU module asks the device)


def tile_class(k):
    """(kc, nch) of rank k: steps = (k + 1) // 2 MFMA steps of two t values, kc the power of two >= steps capped at 64, nch
    the chunks of 2 * kc that k takes (mfx_rec_create)."""
    steps = (k + 1) // 2
    kc = 1
    while kc < steps and kc < 64:
        kc *= 2
    return kc, -(-steps // kc)


def list_size(n_top):
    """(L, lds_sort): the entries of a pair's candidate list, the smallest power of two >= 64 that is >= n_top + 32, and
    whether the flush sorts in LDS (L <= 256) rather than in the list itself."""
    L = 64
    while L < n_top + 32:
        L *= 2
    return L, L <= 256


def probe_slices(nlist, nusers, nprobe, cus):
    """The centroid tiles of every slice of the probe (ivf_probe_dev, topn): about two workgroups per CU, no fewer than four
    tiles a slice, no more than one merge takes.  A trailing 0 is a slice past the last tile: it writes padding."""
    nblkc = -(-nlist // TILE)
    blocks = -(-nusers // USERS_PER_ITEM)
    want = 2 * cus
    s = 1 if blocks >= want else -(-want // blocks)
    s = max(1, min(s, max(1, nblkc // 4), MAX_MERGE // nprobe))
    bps = -(-nblkc // s)
    return [max(0, min(nblkc, (i + 1) * bps) - i * bps) for i in range(s)]


def scan_threads(nlist):
    """(per, full, short, idle): the lists per thread of mfx_ivf_scan, the threads that own `per` lists, the lists of the one
    thread after them (0: there is none) and the threads whose range is clamped to nothing."""
    per = -(-nlist // SCAN_THREADS)
    full, short = divmod(nlist, per)
    return per, full, short, SCAN_THREADS - full - (short > 0)


def work_items(counts):
    """(items per list, first item of every list, total) of the per-list pair counts: ceil(count / 128) each."""
    n = -(-np.asarray(counts, np.int64) // USERS_PER_ITEM)
    off = np.zeros(n.size + 1, np.int64)
    np.cumsum(n, out=off[1:])
    return n, off[:-1], int(off[-1])


def slots_per_launch(nprobe, n_top):
    """Slots of one launch of mfx_rec_query_ivf: the workspace cap over nprobe * L * 8 bytes, rounded down to 128, at least 128."""
    L, _ = list_size(n_top)
    q = WORKSPACE // (nprobe * L * 8)
    return max(USERS_PER_ITEM, q // USERS_PER_ITEM * USERS_PER_ITEM)


def geometry(k, nlist, nusers, nprobe, n_top, cus=CUS, counts=None):
    """What a shape makes the library do, as a namespace: kc, nch; L, lds_sort; slices (the tiles of every probe slice);
    per, full, short, idle (scan); qc (slots per launch) and launches (their sizes); pos_bits (the bits of the widest
    probe position); and, given the pair counts of one launch, wi (work items per list), nwi and the grid bound
    pairs / 128 + min(nlist, pairs) that mfx_ivf_topn is launched with (pairs: all of the launch, padding included)."""
    g = types.SimpleNamespace()
    g.kc, g.nch = tile_class(k)
    g.L, g.lds_sort = list_size(n_top)
    g.slices = probe_slices(nlist, nusers, nprobe, cus)
    g.per, g.full, g.short, g.idle = scan_threads(nlist)
    g.qc = min(nusers, slots_per_launch(nprobe, n_top))
    g.launches = [min(g.qc, nusers - q0) for q0 in range(0, nusers, g.qc)]
    g.pos_bits = (nprobe - 1).bit_length()
    assert g.pos_bits <= POS_BITS and (g.qc - 1) << POS_BITS < 1 << 32
    if counts is not None:
        g.wi, _, g.nwi = work_items(counts)
        pairs = g.launches[0] * nprobe
        g.grid = pairs // USERS_PER_ITEM + min(nlist, pairs)
        assert g.nwi <= g.grid
    return g


# ------------------------------------------------------------------------------------------------ the cases
ROWS = 140
SIZES = [0, 1, 31, 32, 33, 0, 64, 65]     # the forced list sizes of test_gpu_ivf.py; list 8 takes the rest
NONEMPTY = [1, 2, 3, 4, 6, 7, 8]

# a. every tile class: both edges of every KC, nch 1, 2, 3 and 8, odd k for the -0 padding column
TILE_CLASS = {2: (1, 1), 3: (2, 1), 4: (2, 1), 5: (4, 1), 8: (4, 1), 9: (8, 1), 16: (8, 1), 17: (16, 1), 32: (16, 1), 33: (32, 1),
              64: (32, 1), 65: (64, 1), 128: (64, 1), 129: (64, 2), 300: (64, 3), 1024: (64, 8)}
TILE_CASES = [(k, "normal") for k in TILE_CLASS] + [(k, "huge") for k in (4, 16, 128)]
TILE_NPROBE, TILE_NTOP = (1, 3), (10, 100)
# c. candidate-list sizes: both sides of every L, and of the switch from the LDS sort to the sort in global memory
LONG_NTOP = {32: (64, True), 33: (128, True), 96: (128, True), 97: (256, True), 224: (256, True), 225: (512, False),
             512: (1024, False), 1024: (2048, False)}
LONG_NPROBE = (1, 2)
# d. large list counts: nlist -> (cols, k, ((nprobe, n_top), ...))
LARGE = {33: (600, 3, ((1, 10), (3, 10), (33, 10))),
         257: (1000, 4, ((1, 10), (3, 100), (257, 10))),
         1030: (1000, 5, ((1, 10), (64, 100), (1024, 8))),
         65536: (70000, 5, ((3, 10),))}


def forced_assign(rng, cols):
    """An assignment with the list sizes SIZES + [rest], the items of every list scattered over the catalogue."""
    a = np.full(cols, len(SIZES), np.uint32)
    perm = rng.permutation(cols)
    at = 0
    for l, n in enumerate(SIZES):
        a[perm[at:at + n]] = l
        at += n
    return a


def crowded_batch(rng, probes_all, list_ptr, nslots=300, crowd=200):
    """Slot -> user, arbitrary order with duplicates: `crowd` slots are users that probe the most probed non-empty list (so
    that list has more than 128 pairs: several work items), the others any user -> (users, that list)."""
    rows = len(probes_all)
    popular = int(pair_counts(probes_all, list_ptr).argmax())
    fans = np.nonzero((probes_all == popular).any(1))[0]
    users = np.concatenate([rng.choice(fans, crowd), rng.integers(0, rows, nslots - crowd)])
    return users[rng.permutation(nslots)], popular


class Case(types.SimpleNamespace):
    """One model and index of the geometry sweep: W, H, Cn, assign, list_ptr, list_idx, S (every user's exact scores), ex
    (exclusion rows or None), el (their eligibility mask or True), and what the family adds.  probes(nprobe) and
    want(...) are computed once and shared by the host and the GPU module."""

    def probes(self, nprobe):
        if nprobe not in self._probes:
            self._probes[nprobe] = expected_probe(self.W, self.Cn, np.arange(len(self.W)), nprobe)
        return self._probes[nprobe]

    def want(self, name, users, nprobe, n_top, keep=None):
        """expected_query of the batch `users` (an array; `name` is its key in the cache), with the item filter `keep`."""
        key = (name, nprobe, n_top, keep is not None)
        if key not in self._want:
            el = self.el if self.el is True else self.el[users]
            if keep is not None:
                el = el & keep[None, :]
            self._want[key] = expected_query(self.S[users], self.probes(nprobe)[0][users], self.list_ptr, self.list_idx, el, n_top)
        return self._want[key]


def _case(mfx, W, H, Cn, assign, nlist, rng, with_exclusion, **more):
    list_ptr, list_idx = lists_of(assign, nlist)
    rows, cols = len(W), len(H)
    S = chain_scores(W, H, np.arange(rows))
    ex = exclusion(mfx, rng, rows, cols, 10, S) if with_exclusion else None
    el = eligible_mask(ex, np.arange(rows), cols) if with_exclusion else True
    return Case(W=W, H=H, Cn=Cn, assign=assign, nlist=nlist, list_ptr=list_ptr, list_idx=list_idx, S=S, ex=ex, el=el,
                _probes={}, _want={}, **more)


@functools.lru_cache(maxsize=None)
def tile_case(mfx, k, regime, cols=600):
    """a. rows 140 x cols 600 at rank k, nlist = 9 with the forced sizes, exclusion rows, `keep` about half the items, and
    per nprobe a batch of 300 slots in which one list has more than 128 pairs."""
    W, H = regime_factors(regime, ROWS, cols, k, seed=3000 + k)
    _, Cn = regime_factors(regime, ROWS, len(SIZES) + 1, k, seed=4000 + k)
    rng = np.random.default_rng(5000 + k)
    c = _case(mfx, W, H, Cn, forced_assign(rng, cols), len(SIZES) + 1, rng, True, keep=rng.random(cols) < 0.5)
    c.batch = {nprobe: crowded_batch(rng, c.probes(nprobe)[0], c.list_ptr) for nprobe in TILE_NPROBE}
    return c


@functools.lru_cache(maxsize=None)
def boundary_case(mfx, k=8, cols=600):
    """b. the shape of tile_case(8), with users made for the batches of boundary_batches: the centroids of the two empty
    lists 0 and 5 are 3 e0 and 3 e1 and those of the other lists have no component there; per non-empty list l two
    `solo` users along its centroid (they probe l first) and two `trio` users with 4 e0 + 4 e1 added (they probe 0 and 5,
    both empty, and then l: of their three pairs one has work); the last seven users have a NaN row: no list at all."""
    rng = np.random.default_rng(6000)
    W = rng.standard_normal((ROWS, k)).astype(np.float32)
    H = rng.standard_normal((cols, k)).astype(np.float32)
    Cn = rng.standard_normal((len(SIZES) + 1, k)).astype(np.float32)
    Cn[:, :2] = 0.0
    Cn[0], Cn[5] = 0.0, 0.0
    Cn[0, 0], Cn[5, 1] = 3.0, 3.0
    u = 105
    for extra in (0.0, 4.0):
        for l in NONEMPTY:
            for _ in range(2):
                W[u] = 3.0 * Cn[l] / np.linalg.norm(Cn[l])
                W[u, :2] = extra
                u += 1
    W[133:, k // 2] = np.nan
    return _case(mfx, W, H, Cn, forced_assign(rng, cols), len(SIZES) + 1, rng, True)


def boundary_batches(c, nprobe, seed=0):
    """{name: slot -> user} composed from the reference probe so that the non-empty list `l` with the most fans receives
    exactly 128, 129, 256 and 257 pairs (plus 40 slots that do not probe it), `single`: 200 slots whose only pair with
    work goes to l, `one_each`: 257 slots in which every non-empty list gets exactly one pair and 250 slots have none
    -> (batches, l).  Duplicated users are slots of their own."""
    rng = np.random.default_rng(seed + nprobe)
    sizes = np.diff(c.list_ptr.astype(np.int64))
    pr = c.probes(nprobe)[0].astype(np.int64)
    work = [frozenset(int(l) for l in row if l != PAD and sizes[l] > 0) for row in pr]
    fans_of = {l: np.array([u for u, w in enumerate(work) if l in w]) for l in NONEMPTY}
    l = max(NONEMPTY, key=lambda m: len(fans_of[m]))
    others = np.array([u for u, w in enumerate(work) if l not in w])
    only = {m: np.array([u for u, w in enumerate(work) if w == {m}]) for m in NONEMPTY}
    none = np.array([u for u, w in enumerate(work) if not w])
    out = {}
    for n in (128, 129, 256, 257):
        b = np.concatenate([rng.choice(fans_of[l], n), rng.choice(others, 40)])
        out[f"exactly_{n}"] = b[rng.permutation(b.size)]
    out["single"] = rng.choice(only[l], 200)
    b = np.concatenate([[rng.choice(only[m]) for m in NONEMPTY], rng.choice(none, 257 - len(NONEMPTY))])
    out["one_each"] = b[rng.permutation(b.size)]
    return out, l


@functools.lru_cache(maxsize=None)
def long_case(mfx, k=8, cols=1500):
    """c. the forced sizes on 1500 items: list 8 holds 1274, more than 2 L for L <= 512, so the flush that is not the last
    runs; the rising scale of test_one_long_list keeps the threshold admitting items; exclusion rows."""
    rng = np.random.default_rng(7000)
    W = rng.standard_normal((ROWS, k)).astype(np.float32)
    H = (rng.standard_normal((cols, k)) * np.linspace(0.1, 3.0, cols)[:, None]).astype(np.float32)
    Cn = rng.standard_normal((len(SIZES) + 1, k)).astype(np.float32)
    return _case(mfx, W, H, Cn, forced_assign(rng, cols), len(SIZES) + 1, rng, True)


@functools.lru_cache(maxsize=None)
def large_case(mfx, nlist):
    """d. rows 140, k small, nlist lists.  Only the centroids `hot` (two lists) have a component 0, and users 0 .. 2 have
    W[u, 0] = inf: their score is NaN against every other centroid, so they probe exactly two lists; user 3 has a NaN
    row and probes none; the centroids `dead` are NaN and nobody probes them.  nlist = 65536: 60000 lists hold one item
    each and the other 10000 items fall anywhere, so a union is a handful of items; else the items fall anywhere (at
    nlist = 1030 over 1000 items several hundred lists stay empty).  users: every row once and ten again, shuffled."""
    cols, k, _ = LARGE[nlist]
    rng = np.random.default_rng(8000 + nlist)
    W = rng.standard_normal((ROWS, k)).astype(np.float32)
    H = rng.standard_normal((cols, k)).astype(np.float32)
    Cn = rng.standard_normal((nlist, k)).astype(np.float32)
    assign = rng.integers(0, nlist, cols).astype(np.uint32)
    if nlist == 65536:
        assign[:60000] = rng.permutation(nlist)[:60000]
    second = 300 if nlist > 300 else 7                     # (at nlist 1030 and 65536 a list of the probe's second slice)
    assign[:2] = nlist - 1, second                         # the last list (the ragged end of the scan) has an item, and is hot
    hot = np.array([nlist - 1, second])
    Cn[:, 0] = 0.0
    Cn[hot, 0] = [1.5, -0.5]
    dead = np.setdiff1d(rng.choice(nlist, max(4, nlist // 100), replace=False), hot)
    Cn[dead, k - 1] = np.nan
    W[:3, 0] = np.inf
    W[3, 1] = np.nan
    users = np.concatenate([np.arange(ROWS), rng.integers(0, ROWS, 10)])
    return _case(mfx, W, H, Cn, assign, nlist, rng, False, hot=hot, dead=dead, users=users[rng.permutation(users.size)])


CHUNK = types.SimpleNamespace(rows=8300, cols=200, k=3, nlist=8, nprobe=8, n_top=1024, empty=5, nan_users=(8200, 8251, 8299))


@functools.lru_cache(maxsize=None)
def chunk_case():
    """e. the shape of test_user_chunked_launches_equal_query, 8192 slots in the first launch and 108 in the second; list 5
    is empty, and three of the last 108 users have a NaN in their row: all their pairs are padding."""
    g = CHUNK
    rng = np.random.default_rng(9000)
    W = rng.standard_normal((g.rows, g.k)).astype(np.float32)
    H = rng.standard_normal((g.cols, g.k)).astype(np.float32)
    assign = rng.integers(0, g.nlist - 1, g.cols).astype(np.uint32)
    assign[assign >= g.empty] += 1
    Cn = rng.standard_normal((g.nlist, g.k)).astype(np.float32)
    W[list(g.nan_users), 1] = np.nan
    list_ptr, list_idx = lists_of(assign, g.nlist)
    return types.SimpleNamespace(W=W, H=H, Cn=Cn, assign=assign, list_ptr=list_ptr, list_idx=list_idx)
