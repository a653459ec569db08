"""GPU: the three device primitives under every engine step, called on their
own through the debug entry points (include/tropical_hip_debug.h) and compared
with numpy for exact equality:

- the two-stage lexicographic key sort (csrc/sort.hip sort_keys_lex:
  k_lex_runs, k_lex_long, block_bitonic) at every run length its branches
  turn on, and on both sides of the merge-sort limit;
- the single-pass look-back scan (csrc/scan.hip k_scan_lb, common.h
  lb_prefix_rc, engine.cpp lb_begin) at the tile edges, past one look-back
  window, on unaligned input, after a longer launch, near the status word's
  40-bit field and across the wrap of the 22-bit launch epoch;
- the batched fill (scan.hip k_fill / launch_fill) at every head alignment,
  below one 16-byte word, beyond one grid of 16-byte stores, and on ranges of
  very different lengths in one launch.

All inputs are built here from fixed seeds; nothing has a tolerance.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from golden_io import load
from helpers import engine_steps, product_net

pytestmark = pytest.mark.gpu

# constants of the kernels under test (csrc/sort.hip, csrc/scan.hip, engine.cpp)
MERGE_LIMIT = 256 * 1024  # TNP_SORT_MERGE_LIMIT: the two-stage path starts above it
LX_BLOCK = 256            # keys per k_lex_runs block
LX_RMAX = 256             # R is clamped to it
LL_CAP = 8192             # longest run k_lex_long sorts in LDS
TILE = 8192               # elements per k_scan_lb tile
EPOCH_MAX = 0x3FFFFF      # the status word's 22-bit launch epoch
FILL_MAX = 4              # ranges per launch_fill
FILL_GRID_BYTES = 2048 * 256 * 16  # one k_fill grid of 16-byte stores


# ---------------------------------------------------------------------------
# lexicographic key sort
# ---------------------------------------------------------------------------
def run_threshold(R):
    """The run length the two-stage pass ranks in place (R clamped); for the
    one-stage sort (R = 0) the engine's default, so the input keeps its shape."""
    return min(R, LX_RMAX) if R > 0 else 64


def run_lengths(R, n, variant, seed):
    """Run lengths summing to n: every length a branch of the sort turns on,
    three times each in seeded random order among filler runs of 1-4 keys,
    then runs placed at chosen positions of the lo-sorted array."""
    rng = np.random.default_rng(seed)
    Rq = run_threshold(R)
    special = {1, 2, 3, 255, 256, 257, 300, 1000, LL_CAP, LL_CAP + 1, 20000}
    for r in {R, Rq}:
        special |= {r - 1, r, r + 1, r + 2, 2 * r + 3}
    special = sorted(x for x in special if x > 0)
    head, tail = [], []
    if variant == "edges":      # a long run at position 0 and one ending at n
        head, tail = [Rq + 1], [Rq + 1]
    elif variant == "long_first":  # the run beyond the LDS first
        head = [20000]
    placed = []                 # pads of single keys bring the position to 255 (mod 256)

    def pad_to(pos, want):
        k = (want - pos) % LX_BLOCK
        placed.extend([1] * k)
        return pos + k

    pos = sum(head)
    for length in (Rq, Rq + 1):  # a ranked run and a listed run across a block edge
        pos = pad_to(pos, LX_BLOCK - 1)
        placed.append(length)
        pos += length
    pos = pad_to(pos, LX_BLOCK - 3)  # a run ending at a block edge
    placed.append(3)
    pos += 3
    body = special * 3
    room = n - pos - sum(body) - sum(tail)
    assert room > 0
    filler = rng.integers(1, 5, size=room)  # more than needed; cut to fit
    cut = int(np.searchsorted(np.cumsum(filler), room, side="right"))
    filler = list(filler[:cut])
    rest = room - sum(filler)
    if rest:
        filler.append(rest)
    mixed = np.array(body + filler, dtype=np.int64)
    rng.shuffle(mixed)
    lengths = np.array(head + placed + list(mixed) + tail, dtype=np.int64)
    assert lengths.sum() == n and (lengths > 0).all()
    return lengths, special


def keys_from_runs(lengths, nb, seed):
    """Unique keys lo << nb | hi, shuffled: run r has lengths[r] keys of one
    lo (ascending with r, the first 0 and the last 2^nb - 1), their hi
    distinct and spread over [0, 2^nb)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    n, runs = int(lengths.sum()), len(lengths)
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    gap = rng.integers(1, max((1 << nb) // runs, 1) + 1, size=runs, dtype=np.int64)
    lo = np.cumsum(gap) - gap[0]
    if runs > 1:
        lo[-1] = (1 << nb) - 1
    assert lo[-1] < (1 << nb) and (np.diff(lo) > 0).all()
    start = np.cumsum(lengths) - lengths
    rid = np.repeat(np.arange(runs), lengths)
    # a random order inside every run: key i takes slot[i] of its run's
    # lengths[r] equal strides of [0, 2^nb), at a random offset in the stride
    order = np.lexsort((rng.random(n), rid))
    slot = np.empty(n, dtype=np.int64)
    slot[order] = np.arange(n) - start[rid[order]]
    stride = (1 << nb) // lengths[rid]
    assert (stride > 0).all()
    hi = slot * stride + (rng.random(n) * stride).astype(np.int64)
    assert (hi >= 0).all() and (hi < (1 << nb)).all()
    keys = (lo[rid].astype(np.uint64) << np.uint64(nb)) | hi.astype(np.uint64)
    return keys[rng.permutation(n)]


def runs_of(sorted_keys, nb):
    """(start, length) of every run of equal lo in the lo-sorted array."""
    lo = sorted_keys >> np.uint64(nb)
    start = np.concatenate([[0], np.flatnonzero(lo[1:] != lo[:-1]) + 1])
    return start, np.diff(np.concatenate([start, [len(lo)]]))


def device_lex_sort(keys, nb, R, dev):
    """sort_keys_lex on a device copy of `keys`; the copy must come back
    untouched."""
    from tropical import _hip
    k = torch.from_numpy(keys.view(np.int64)).to(dev)
    before = k.clone()
    out = torch.empty_like(k)
    _hip.check(_hip.lib().tnp_debug_sort_keys_lex(_hip.ptr(k), k.shape[0], nb, R, _hip.ptr(out),
                                                  C.c_void_p(_hip.stream_ptr(dev))), "tnp_debug_sort_keys_lex")
    assert torch.equal(k, before), "the caller's keys were modified"
    return out.cpu().numpy().view(np.uint64)


def check_keys(keys, nb):
    assert len(np.unique(keys)) == len(keys), "the rank pass needs unique keys"
    if 2 * nb < 64:
        assert not (keys >> np.uint64(2 * nb)).any()


LEX_PAIRS = [(20, 64), (20, 1), (20, 2), (20, 256), (20, 1000), (20, 0), (19, 64), (31, 64)]


@pytest.mark.parametrize("variant", ["mixed", "edges", "long_first"])
@pytest.mark.parametrize("nb,R", LEX_PAIRS)
def test_lex_sort_run_structure(cuda, nb, R, variant):
    """n just above the merge limit, so R > 0 takes the two-stage path; runs
    of every length at which k_lex_runs / k_lex_long change branch: 1..3,
    around R (ranked in place up to R, listed from R + 1), around the 256-key
    block, around LL_CAP (LDS up to it, in place in memory beyond), 20000.
    (20, 1000): R clamped to LX_RMAX; (20, 0): the one-stage sort of the same
    input; (31, 64): both halves use their top bit."""
    n = 300_007
    Rq = run_threshold(R)
    lengths, special = run_lengths(R, n, variant, seed=1000 * nb + R)
    keys = keys_from_runs(lengths, nb, seed=7 + 1000 * nb + R)
    assert len(keys) == n > MERGE_LIMIT
    check_keys(keys, nb)
    want = np.sort(keys)
    # what the construction must contain, read off the lo-sorted array
    start, length = runs_of(want, nb)
    assert np.array_equal(length, lengths)
    assert set(special) <= set(length.tolist())
    assert {Rq - 1, Rq, Rq + 1, Rq + 2, 2 * Rq + 3, LL_CAP, LL_CAP + 1, 20000} - {0} <= set(length.tolist())
    assert ((length == Rq) & (start % LX_BLOCK == LX_BLOCK - 1)).any()
    assert ((length == Rq + 1) & (start % LX_BLOCK == LX_BLOCK - 1)).any()
    assert ((start + length) % LX_BLOCK == 0).any()
    if variant == "edges":
        assert length[0] == Rq + 1 and length[-1] == Rq + 1
    if variant == "long_first":
        assert length[0] == 20000
    top = np.uint64(1 << (nb - 1))
    assert ((want >> np.uint64(nb)) & top).any() and (want & top).any()
    got = device_lex_sort(keys, nb, R, cuda)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [0, 1, 2, MERGE_LIMIT, MERGE_LIMIT + 1])
def test_lex_sort_both_sides_of_the_merge_limit(cuda, n):
    """Up to TNP_SORT_MERGE_LIMIT keys sort_keys_lex is the one-stage sort on
    all 2 nb bits, one key more takes the two-stage path: both must sort, a
    run of 100 (above R = 64) inside."""
    nb, R = 20, 64
    rng = np.random.default_rng(n + 11)
    if n > 100:
        filler = rng.integers(1, 5, size=n)
        cut = int(np.searchsorted(np.cumsum(filler), n - 100, side="right"))
        filler = list(filler[:cut])
        rest = n - 100 - sum(filler)
        lengths = filler[: cut // 2] + [100] + filler[cut // 2:] + ([rest] if rest else [])
    else:
        lengths = [1] * n
    keys = keys_from_runs(lengths, nb, seed=n + 12)
    assert len(keys) == n
    check_keys(keys, nb)
    want = np.sort(keys)
    if n > 100:
        assert 100 in runs_of(want, nb)[1]
    got = device_lex_sort(keys, nb, R, cuda)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------
# look-back scan
# ---------------------------------------------------------------------------
def fresh_engine(dev, spin):
    from tropical._engine import Engine
    eng = Engine(dev)
    eng.debug_lb(spin)
    return eng


def scan_ref(x):
    """(exclusive prefix sums, total) in int64."""
    x = np.asarray(x)
    if len(x) == 0:
        return np.zeros(0, dtype=np.int64), 0
    return np.concatenate([[0], np.cumsum(x, dtype=np.int64)[:-1]]), int(x.sum(dtype=np.int64))


def check_scan(eng, x, dev, what=""):
    """One scan of the host int32 array x on the engine; exact against numpy."""
    d = torch.from_numpy(x).to(dev)
    out, total = eng.debug_scan(d)
    want, want_total = scan_ref(x)
    assert total == want_total, what
    assert np.array_equal(out.cpu().numpy(), want), what


def tiles(n):
    return (n + TILE - 1) // TILE


SCAN_N = [0, 1, 31, 32, 33, TILE - 1, TILE, TILE + 1, 64 * TILE, 64 * TILE + 1, 65 * TILE + 1, 130 * TILE + 5]


@pytest.mark.parametrize("spin", [-1, 0])
@pytest.mark.parametrize("n", SCAN_N)
def test_scan_tile_edges(cuda, n, spin):
    """n around a thread's 32 elements, around one tile, at 64 tiles (one
    look-back window), one tile and one window more, and 130 tiles; spin 0
    sends every unpublished predecessor through the recompute path, which
    must then really run."""
    eng = fresh_engine(cuda, spin)
    x = np.random.default_rng(n + 1).integers(0, 1001, size=n, dtype=np.int32)
    check_scan(eng, x, cuda)
    recomputes = eng.debug_lb()
    if spin == 0 and tiles(n) > 1:
        assert recomputes > 0


@pytest.mark.parametrize("spin", [-1, 0])
def test_scan_after_a_longer_launch(cuda, spin):
    """130 tiles, then 3 tiles of other data on the same engine: the records
    the longer launch left (another epoch) must not be taken."""
    eng = fresh_engine(cuda, spin)
    rng = np.random.default_rng(5)
    check_scan(eng, rng.integers(0, 1001, size=130 * TILE + 5, dtype=np.int32), cuda)
    check_scan(eng, rng.integers(0, 1001, size=2 * TILE + 77, dtype=np.int32), cuda)


@pytest.mark.parametrize("spin", [-1, 0])
def test_scan_unaligned_input(cuda, spin):
    """An input 4 bytes past a 16-byte boundary takes the scalar loads."""
    eng = fresh_engine(cuda, spin)
    n = 3 * TILE + 7
    x = np.random.default_rng(6).integers(0, 1001, size=n + 1, dtype=np.int32)
    d = torch.from_numpy(x).to(cuda)[1:]
    assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    out, total = eng.debug_scan(d)
    want, want_total = scan_ref(x[1:])
    assert total == want_total
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("spin", [-1, 0])
def test_scan_fills_the_40_bit_field(cuda, spin):
    """2^20 counts of 2^20 - 1: the last records hold almost 2^40, the most
    the status word's value field is asked to hold."""
    eng = fresh_engine(cuda, spin)
    x = np.full(1 << 20, (1 << 20) - 1, dtype=np.int32)
    d = torch.from_numpy(x).to(cuda)
    out, total = eng.debug_scan(d)
    assert total == (1 << 40) - (1 << 20)
    assert np.array_equal(out.cpu().numpy(), scan_ref(x)[0])


@pytest.mark.parametrize("last_before_wrap", ["70_tiles", "3_tiles"])
@pytest.mark.parametrize("spin", [-1, 0])
def test_scan_epoch_wrap(cuda, spin, last_before_wrap):
    """The 22-bit launch epoch wraps after 2^22 launches of a chain; lb_begin
    then clears the records, because the epochs start again at 1 and records
    of the engine's first launches may still carry those.  A's 70 records
    carry epoch 1; with the epoch preset two short of the wrap, the next
    scans run at epochs 0x3FFFFF, 1 (the wrap) and 2, the last two of B over
    70 tiles.  70_tiles: the scan before the wrap is B's as well -- the epoch
    sequence, but that scan rewrites all 70 records, so none of A's is left
    for the wrap to meet.  3_tiles: it is a shorter one, A's records of tiles
    3..69 survive it, and without the clear the scan at the wrap (the second
    after the preset) takes them as inclusive prefixes of its own launch."""
    eng = fresh_engine(cuda, spin)
    rng = np.random.default_rng(8)
    n = 70 * TILE
    a = rng.integers(0, 1001, size=n, dtype=np.int32)
    b = rng.integers(0, 1001, size=n, dtype=np.int32)
    c = b if last_before_wrap == "70_tiles" else rng.integers(0, 1001, size=2 * TILE + 9, dtype=np.int32)
    check_scan(eng, a, cuda)
    assert eng.debug_lb_epoch(0) == 1
    assert eng.debug_lb_epoch(0, set=EPOCH_MAX - 1) == 1
    for x, epoch in ((c, EPOCH_MAX), (b, 1), (b, 2)):
        check_scan(eng, x, cuda, f"the scan at epoch {epoch:#x}")
        assert eng.debug_lb_epoch(0) == epoch


def test_epoch_wrap_under_an_extraction(cuda):
    """The wrap in the middle of a real run: synth24's lattice steps once (both
    chains' records now carry low epochs), the epochs preset three short of
    the wrap, and the steps again -- every state must be the golden's.  Chain
    0 also serves the ticketed kernels, whose ticket base the wrap resets."""
    from tropical._engine import engine_for
    d = load("synth24")
    net = product_net(d, cuda)
    eng = engine_for(net)
    before = [eng.debug_lb_epoch(w) for w in (0, 1)]
    eng.lattice(keep_all=True)
    engine_steps(eng, record=False)
    launches = [eng.debug_lb_epoch(w) - before[w] for w in (0, 1)]
    assert launches[0] >= 4, launches  # the second run crosses the wrap on chain 0
    for w in (0, 1):
        eng.debug_lb_epoch(w, set=EPOCH_MAX - 3)
    eng.lattice(keep_all=True)
    got = engine_steps(eng)
    assert len(got) == len(d["step_sha"])
    for g, V, E, s in zip(got, d["step_V"], d["step_E"], d["step_sha"]):
        assert (g[0], g[1], g[2]) == (V, E, s)
    for w in (0, 1):
        if launches[w] >= 4:  # (a chain this run never launches on keeps its preset)
            assert 1 <= eng.debug_lb_epoch(w) < (1 << 16)


# ---------------------------------------------------------------------------
# batched fill
# ---------------------------------------------------------------------------
GUARD = 64


class FillRange:
    """`length` bytes at `offset` past a 16-byte boundary, 64 guard bytes on
    either side, in a device tensor of its own pre-filled with a pattern."""

    def __init__(self, dev, offset, length, byte, seed=0):
        size = GUARD + offset + length + GUARD
        self.host = ((np.arange(size, dtype=np.int64) * 7 + seed) % 251).astype(np.uint8)
        self.dev = torch.from_numpy(self.host).to(dev)
        assert self.dev.data_ptr() % 16 == 0
        self.first, self.length, self.byte = GUARD + offset, length, byte
        self.ptr = self.dev.data_ptr() + self.first

    def want(self):
        w = self.host.copy()
        w[self.first:self.first + self.length] = self.byte
        return w

    def got(self):
        return self.dev.cpu().numpy()


def device_fill(ops, dev):
    """One tnp_debug_fill call on (pointer, bytes, value) triples; returns rc."""
    from tropical import _hip
    k = len(ops)
    ptrs = (C.c_void_p * max(k, 1))(*[p for p, _, _ in ops])
    sizes = (C.c_uint64 * max(k, 1))(*[n for _, n, _ in ops])
    vals = (C.c_uint32 * max(k, 1))(*[b for _, _, b in ops])
    rc = _hip.lib().tnp_debug_fill(ptrs, sizes, vals, k, C.c_void_p(_hip.stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    return rc


def test_fill_every_alignment_and_short_length(cuda):
    """Head alignments 0..15 x lengths below, at and above one and two 16-byte
    words, and a body with both ends ragged: the range set, every other byte
    (the guards included) as before."""
    for offset in range(16):
        for length in (0, 1, 15, 16, 17, 31, 32, 33, 4096 + 5):
            r = FillRange(cuda, offset, length, 0xA5, seed=offset + length)
            assert device_fill([(r.ptr, length, 0xA5)], cuda) == 0
            assert np.array_equal(r.got(), r.want()), (offset, length)


def test_fill_grid_stride(cuda):
    """More 16-byte words than one grid of k_fill stores: the grid-stride
    body, with a ragged head and tail."""
    length = FILL_GRID_BYTES + 48 + 7
    assert length > FILL_GRID_BYTES
    r = FillRange(cuda, 3, length, 0x3C)
    assert device_fill([(r.ptr, length, 0x3C)], cuda) == 0
    assert np.array_equal(r.got(), r.want())


def test_fill_four_ranges_of_different_lengths(cuda):
    """One launch, its grid sized by the largest range; the small ranges'
    heads and tails are block 0's.  Null and empty ranges among them are
    skipped and do not count towards FILL_MAX."""
    spec = [(1, 5, 0x11), (15, 17, 0xEE), (8, FILL_GRID_BYTES + 9, 0x5A), (0, 1000, 0x80)]
    rs = [FillRange(cuda, off, n, b, seed=i) for i, (off, n, b) in enumerate(spec)]
    skipped = FillRange(cuda, 0, 32, 0xFF, seed=9)
    ops = [(r.ptr, r.length, r.byte) for r in rs]
    ops = [ops[0], (None, 10, 0x77), ops[1], (skipped.ptr, 0, 0xFF), ops[2], ops[3]]
    assert device_fill(ops, cuda) == 0
    for r in rs:
        assert np.array_equal(r.got(), r.want())
    assert np.array_equal(skipped.got(), skipped.host)
    # nothing but skipped ranges: no launch, no change
    assert device_fill([(None, 10, 0x77), (skipped.ptr, 0, 0xFF)], cuda) == 0
    assert device_fill([], cuda) == 0
    assert np.array_equal(skipped.got(), skipped.host)


def test_fill_refuses_a_fifth_range(cuda):
    from tropical import _hip
    rs = [FillRange(cuda, i, 100 + i, 0xC0 + i, seed=i) for i in range(FILL_MAX + 1)]
    assert device_fill([(r.ptr, r.length, r.byte) for r in rs], cuda) == -1
    assert f"launch_fill: more than {FILL_MAX} ranges" in _hip.lib().tnp_last_error().decode()
    for r in rs:
        assert np.array_equal(r.got(), r.host)
