"""Every route of the batch-walking row kernels (csrc/specwalk.hip: spec_mid_walk, spec_gradh_walk, sum_parts_kernel behind
ops.spectral_apply) against torch.fft + einsum in float64 on the CPU, with the knobs that choose the route SET BY THE TEST:
the workgroup count and partition of the forward kernel, the batch slices of the backward kernel, the cache-policy mask.
On a card they are all derived from the CU count, so without this file a partitioned card -- or a change of walk_wgs /
fl_spec_gradh_slices -- moves the whole suite onto other paths of these kernels unnoticed.

Routes, and the test that launches each:
  partition of spec_mid_walk (fl_spec_walk_workgroups + fl_spec_walk_partition)
    a workgroup that walks through a complete row pair into a third one (drain, refill, a full segment, drain), ranges that
    start / end on a self-mirrored row pair or in the middle of one, one-unit and empty ranges, a grid that is no multiple
    of 8 (no XCD reordering: 1, 3) ....................................... test_partitions (host pins: test_plans_and_partitions)
    bounds == nullptr, the equal-count split of a graph capture with a cold cache ............................ test_null_bounds
    segments shorter than _WALK_MIN_BATCH (one, two, three units per row pair) ............................. test_short_batches
  batch slices of spec_gradh_walk (fl_spec_gradh_slices) and fl_sum_parts_c64
    slices of one item (prologue + epilogue only), uneven slices (1 + 2, 2 + 3 items), up to 7 partial planes, DEPTH 2
    (8 -> 8) and DEPTH 1, NSC 2 and NSC 1 (two output channels) ............................................. test_batch_slices
    mode 15 (NSC = 1 at 8 -> 8 channels, 240-bin rows) ........................................................ test_mode_15
    out_scale multiplied into every partial plane (ops.mean_square as the objective) ............ test_sliced_planes_take_out_scale
  instantiations: 9 channel pairs x 2 row lengths of both kernels, each forward instantiation also as the adjoint of its
    transpose; odd L1 at 240- and at 256-bin rows ....................................................... test_every_instantiation
  policy bits 4-9 (dma16sp<true>, plain stores ...) and 14 (item order) of fl_set_stream_policy ............... test_policy_bits

Reference: torch.fft.rfft -> einsum("fmn,bfn->bfm") -> torch.fft.irfft and its autograd in float64 on the CPU; the inputs are
drawn in float32 and widened.  Limits: the project's float32 limits (conftest.check_close: relative l2 below 1e-5, max-norm
below 1e-4), applied PER BLOCK as well as to whole tensors: y and gx are taken to bins (torch.fft.rfft, float64, CPU), natural
bin k belongs to row pair min(k % L1, L1 - k % L1); every (batch item, row pair) block of y and gx and every row pair of gH
is held to the limits on its own, the self-mirrored row pairs (r = 0 with DC and Nyquist; r = L1 / 2 for even L1) in an
assertion of their own.  A unit that is wrong is named, and is not averaged away.  The allocator is poisoned (_poison): its
cache is emptied and NaN blocks of the sizes of S, S2, Xp, the partial planes and the summed plane are handed to it, so that
a unit or plane that no workgroup writes reads NaN rather than what the previous run of a ladder left there.  This rests on
the allocator reusing those blocks; it is a precaution, not a proof.

Bit-identities asserted (torch.equal) -- a unit's arithmetic reads only its own rows, its row pair's response and the tables,
so none of these may depend on which workgroup runs it or with which cache policy:
  y, gx, gH across every workgroup count and the null-bounds split (slice count fixed);
  y, gx across slice counts, modes and item orders; y, gx, gH across policy bits 4-9.
gH across slice counts, mode 15 and bit 14 sums in another order: compared with float64 per row pair.
Measured on an MI355X: every one of these identities holds, and the worst single block of any case is at l2 2.9e-7, max-norm
4.6e-7 (whole tensors 2.1e-7 .. 2.7e-7, as walk_shapes/* of test_round4): no class of blocks comes near the limit, so none
is given an allowance for arithmetic it shares with the one-item row kernel.

What the launch records cannot show: spec_gradh_walk has one span name for NSC 1 and NSC 2, and the policy bits change no
name at all.  test_mode_15 therefore asserts the one effect of mode 15 that a host entry shows (fl_spec_gradh_slices counts
one workgroup per row pair instead of two); that the mode and the policy bits reach the kernels' dispatch is read in
csrc/specwalk.hip (g_walk_nsc in FL_GRADH_ROWS, a.pol = stream_policy()), not observed here: test_mode_15 and test_policy_bits
show that the results are right and identical WHATEVER these knobs select, not which instantiation ran.

The plan of 36000 (75 x 240, the one 240-bin length with a column length no test launches) is pinned by the host test only."""
import ctypes
import functools
from collections import namedtuple

import pytest
import torch

from conftest import cc

TOL, MAX_TOL = 1e-5, 1e-4
# nfft -> (L1, L2): the smallest lengths with 240- / 256-bin rows; column lengths 50, 125, 128 are launched by other tests too
# (36000: plan only)
PLANS = {24000: (50, 240), 60000: (125, 240), 65536: (128, 256), 64000: (125, 256), 36000: (75, 240)}
CHANNELS = (2, 4, 8)
WGS_LADDER = (1, 3, 8, 16, 40, 1 << 20)        # the last: clamped to the units (rounded down to a multiple of 8)
CU_256 = 256                                   # the workgroup count a 256-CU card would start from
# fl_spec_walk_partition at (24000, batch 4): workgroups -> bounds
PINNED_BOUNDS = {
    3: [0, 36, 71, 104],
    8: [0, 13, 26, 39, 52, 65, 78, 91, 104],
}


def _lib():
    from flamo_amd import _lib as m
    return m.lib()


def _plan(nfft):
    l1, l2 = ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib().fl_spec_plan(nfft, ctypes.byref(l1), ctypes.byref(l2))
    return rc, (l1.value, l2.value)


def _grid(nfft, B, wgs):
    """the forward kernel's grid with the workgroup count pinned to `wgs` (needs no device)"""
    L = _lib()
    assert L.fl_debug_set_walk(1, wgs, 0, None) == 0
    try:
        return int(L.fl_spec_walk_workgroups(nfft, B))
    finally:
        L.fl_debug_set_walk(1, 0, 0, None)


def _bounds(nfft, B, n_wg):
    host = (ctypes.c_int * (n_wg + 1))()
    assert _lib().fl_spec_walk_partition(nfft, B, n_wg, host) == 0
    return list(host)


def _equal_counts(nfft, B, n_wg):
    """the kernel's own split when it is handed no bounds (spec_mid_walk: Utot * w / G)"""
    U = (PLANS[nfft][0] // 2 + 1) * B
    return [U * w // n_wg for w in range(n_wg + 1)]


def _self_mirrored(nfft):
    L1 = PLANS[nfft][0]
    return {0} | ({L1 // 2} if L1 % 2 == 0 else set())


def _features(nfft, B, bounds):
    """what the ranges of a partition contain, as a set of names"""
    P, sm, out = PLANS[nfft][0] // 2 + 1, _self_mirrored(nfft), set()
    assert bounds[0] == 0 and bounds[-1] == P * B and all(a <= b for a, b in zip(bounds, bounds[1:]))
    for lo, hi in zip(bounds, bounds[1:]):
        if lo == hi:
            out.add("empty")
            continue
        if hi - lo == 1:
            out.add("one-unit")
        r_lo, r_hi = lo // B, (hi - 1) // B
        if r_lo in sm:
            out.add("starts-self-mirrored")
        if r_hi in sm:
            out.add("ends-self-mirrored")
        if lo % B and hi % B:
            out.add("mid-to-mid")
        if any(r not in sm and lo < r * B and hi > (r + 1) * B for r in range(r_lo + 1, r_hi)):
            out.add("whole-pair-between-neighbours")
        if r_hi - r_lo >= 2:
            out.add("third-row-pair")
    return out


# ----------------------------------------------------------------------------- 1. host: plans and partitions
def test_plans_and_partitions():
    """fl_spec_plan for the lengths of this file and fl_spec_walk_partition for the (nfft, batch, workgroups) triples of the GPU
    tests (no GPU): the ranges contain what those tests are written for."""
    for nfft, want in PLANS.items():
        assert _plan(nfft) == (0, want), nfft
    # the grids the ladder pins: 1 and 3 take the branch without XCD reordering, the last rung is clamped to the units
    assert [_grid(24000, 4, w) for w in WGS_LADDER] == [1, 3, 8, 16, 40, 104]
    assert [_grid(24000, 5, w) for w in WGS_LADDER] == [1, 3, 8, 16, 40, 128]
    assert [_grid(65536, 4, w) for w in WGS_LADDER] == [1, 3, 8, 16, 40, 256]
    assert [_grid(65536, 5, w) for w in WGS_LADDER] == [1, 3, 8, 16, 40, 320]
    assert _grid(24000, 5, CU_256) == 128 and _grid(65536, 5, CU_256) == 256 and _grid(60000, 5, CU_256) == 256
    for g, want in PINNED_BOUNDS.items():
        assert _bounds(24000, 4, g) == want, g
    b16, b40, b104 = _bounds(24000, 4, 16), _bounds(24000, 4, 40), _bounds(24000, 4, 104)
    lens16 = [b - a for a, b in zip(b16, b16[1:])]
    assert min(lens16) == 3 and max(lens16) == 8
    assert sum(a == b for a, b in zip(b40, b40[1:])) == 2          # 38 ranges, two surplus workgroups
    assert b104 == list(range(105))                                  # one unit each: [0, 1) ends on row pair 0 (DC / Nyquist),
    assert 100 // 4 == 25 in _self_mirrored(24000)                   # [100, 101) starts on row pair 25 = L1 / 2
    # every feature is present at each (length, batch) of test_partitions, over the ladder
    for nfft in (24000, 65536):
        for B in (4, 5):
            seen = {}
            for w in WGS_LADDER:
                g = _grid(nfft, B, w)
                seen[g] = _features(nfft, B, _bounds(nfft, B, g))
            assert "whole-pair-between-neighbours" in seen[1] & seen[3] & seen[8], (nfft, B)
            assert "third-row-pair" in seen[16] and "mid-to-mid" in seen[16], (nfft, B)
            allf = set().union(*seen.values())
            assert {"starts-self-mirrored", "ends-self-mirrored", "one-unit", "mid-to-mid"} <= allf, (nfft, B, allf)
            if nfft == 24000:
                assert "empty" in seen[40], (nfft, B)
    assert "mid-to-mid" in _features(24000, 4, PINNED_BOUNDS[8])                      # [13, 26): units 1 of row pair 3 .. 1 of 6
    # the equal-count split of test_null_bounds cuts row pairs in the middle and differs from the cost-balanced one
    for g in (3, 16):
        eq = _equal_counts(24000, 5, g)
        assert eq != _bounds(24000, 5, g) and "mid-to-mid" in _features(24000, 5, eq)
    # test_short_batches: with one item per row pair every segment is one unit, and a workgroup still crosses row pairs
    for B in (1, 2, 3):
        assert _grid(24000, B, 8) == 8 and "third-row-pair" in _features(24000, B, _bounds(24000, B, 8))


# ----------------------------------------------------------------------------- reference
_Data = namedtuple("_Data", "nfft NI NO B x H c objective gHr Yr GXr rp P")


@functools.lru_cache(maxsize=None)      # every case of the file keeps its entry (about 1 GB in all): most share their data
def _data(nfft, NI, NO, B, seed=0, objective="dot"):
    """float32 inputs (CPU) and the float64 results for the objective sum(y c) ("dot") or mean(y^2) ("mean_square"): gH, and y
    and gx in bins (Yr, GXr: the time-domain references are their inverse transforms, _time); rp: the row pair of every
    natural bin"""
    g = torch.Generator().manual_seed(1000 * seed + nfft % 977 + 10 * NI + NO + 100 * B)
    M, L1 = nfft // 2 + 1, PLANS[nfft][0]
    x = torch.randn(B, nfft, NI, generator=g)
    H = torch.randn(M, NO, NI, dtype=torch.complex64, generator=g) / NI ** 0.5
    c = torch.randn(B, nfft, NO, generator=g)
    xr = x.double().requires_grad_(True)
    Hr = H.to(torch.complex128).requires_grad_(True)
    yr = torch.fft.irfft(torch.einsum("fmn,bfn->bfm", Hr, torch.fft.rfft(xr, n=nfft, dim=1)), n=nfft, dim=1)
    loss = (yr * c.double()).sum() if objective == "dot" else (yr ** 2).mean()
    gxr, gHr = torch.autograd.grad(loss, [xr, Hr])
    k1 = torch.arange(M) % L1
    return _Data(nfft, NI, NO, B, x, H, c, objective, gHr, torch.fft.rfft(yr.detach(), dim=1), torch.fft.rfft(gxr, dim=1),
                 torch.minimum(k1, L1 - k1), L1 // 2 + 1)


def _time(Z, nfft):
    return torch.fft.irfft(Z, n=nfft, dim=1)


def _block_errors(got, ref, rp, P):
    """got, ref: (lead, M, C) complex128 -> per (lead, row pair): l2 error / l2 norm, max error / max magnitude"""
    lead = got.shape[0]
    d = (got - ref).abs()
    a = ref.abs()
    idx = rp.view(1, -1).expand(lead, -1)
    num = torch.zeros(lead, P, dtype=torch.float64).scatter_add_(1, idx, (d * d).sum(-1))
    den = torch.zeros(lead, P, dtype=torch.float64).scatter_add_(1, idx, (a * a).sum(-1))
    dmx = torch.zeros(lead, P, dtype=torch.float64).scatter_reduce_(1, idx, d.amax(-1), "amax")
    amx = torch.zeros(lead, P, dtype=torch.float64).scatter_reduce_(1, idx, a.amax(-1), "amax")
    return (num / den).sqrt(), dmx / amx


def _check_blocks(what, got, ref, d):
    """every (batch item, row pair) block within the limits; the self-mirrored row pairs first, in their own assertion"""
    l2, mx = _block_errors(got, ref, d.rp, d.P)

    def worst(cols):
        e, m = l2[:, cols], mx[:, cols]
        bad = ~((e < TOL) & (m < MAX_TOL))              # (a NaN is bad)
        i = int(torch.argmax(torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)))
        b, j = divmod(i, len(cols))
        return bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} blocks out; worst (item {b}, row pair {cols[j]}): " \
                                f"l2 {e[b, j].item():.3e} max {m[b, j].item():.3e}"
    sm = sorted(_self_mirrored(d.nfft))
    print(f"[blocks] {what}: worst block l2 {l2.max().item():.3e}  max {mx.max().item():.3e}  (self-mirrored l2 {l2[:, sm].max().item():.3e})")
    bad, msg = worst(sm)
    assert not bad, "self-mirrored " + msg
    bad, msg = worst([r for r in range(d.P) if r not in sm])
    assert not bad, "interior " + msg
    return l2.max().item()


def _check(tag, res, d, whole=True, only=("y", "gx", "gH")):
    """a result (y, gx, gH) on the CPU against the float64 reference: per block, and one whole-tensor record each"""
    y, gx, gH = res
    if "y" in only:
        assert y.shape == (d.B, d.nfft, d.NO) and y.dtype == torch.float32
        _check_blocks(tag + "y", torch.fft.rfft(y.double(), dim=1), d.Yr, d)
    if "gx" in only:
        assert gx.shape == d.x.shape and gx.dtype == torch.float32
        _check_blocks(tag + "gx", torch.fft.rfft(gx.double(), dim=1), d.GXr, d)
    if "gH" in only:
        assert gH.shape == d.gHr.shape and gH.dtype == torch.complex64
        M = d.gHr.shape[0]
        _check_blocks(tag + "gH", gH.to(torch.complex128).reshape(1, M, -1), d.gHr.reshape(1, M, -1), d)
    if whole:
        for k, a, b in (("y", y, d.Yr), ("gx", gx, d.GXr), ("gH", gH, d.gHr)):
            if k in only:
                cc(tag + k, a, b if k == "gH" else _time(b, d.nfft), TOL)


def _same(tag, res, base, d, only=("y", "gx", "gH")):
    """bit-identical to `base`; where it is not, the float64 comparison names the unit before the identity fails"""
    names = ("y", "gx", "gH")
    diff = [k for k, a, b in zip(names, res, base) if k in only and not torch.equal(a, b)]
    if diff:
        _check(tag, res, d, whole=False, only=diff)
    assert not diff, f"{tag}: {diff} not bit-identical to the base run (within the float64 limits per block)"


# ----------------------------------------------------------------------------- one run with its knobs pinned
def _poison(dev, d, slices):
    """NaN blocks of the sizes the operator allocates -- S / S2 / S3 of the adjoint, Xp, the partial planes, the summed plane,
    two copies each -- handed to the caching allocator and freed, as _poison of tests/test_cascade_oracle.py does: the
    operator's buffers of the same sizes are carved from them, in the allocator's small pool (requests up to 1 MiB: the
    two-channel shapes, one-item batches) as well as in the large one.  The cache is emptied first: the holes the previous
    run of a ladder left have the same sizes and hold that run's, right, values, and the allocator would prefer them.
    One NaN block larger than a whole forward + backward pass goes in front, so that what the large pool hands out beyond
    the exact sizes is NaN as well.  A hole that a temporary of THIS pass frees (the response's transposed copy, a scratch
    array) can still be taken in place of a NaN block: an unwritten unit then reads that temporary, not NaN"""
    from flamo_amd import ops
    half, Pm = d.nfft // 2, ops._pitch(d.nfft // 2 + 1)
    scratch, plane = d.B * half * max(d.NI, d.NO) * 8, d.NO * d.NI * Pm * 8
    xp = int(_lib().fl_spec_walk_spectrum_elems(d.nfft, d.B, d.NI)) * 8
    sizes = [d.B * half * d.NI * 8, d.B * half * d.NO * 8, xp, slices * plane, plane]

    def nan_block(nbytes):
        return torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    big = nan_block(16 * scratch + 3 * xp + (slices + 6) * plane)
    torch.cuda.synchronize(dev)
    del big
    blocks = [nan_block(n) for n in sizes for _ in range(2)]
    torch.cuda.synchronize(dev)
    del blocks


def _run(dev, d, wgs, slices=1, mode=1, min_batch=None, null_bounds=False):
    """ops.spectral_apply forward + backward with the forward kernel's workgroups, the backward kernel's slices and mode pinned;
    asserts the launches; every knob is back at its default afterwards.  -> (y, gx, gH) on the CPU"""
    from flamo_amd import ops
    L = _lib()
    nfft, NI, NO, B = d.nfft, d.NI, d.NO, d.B
    keep = ops._WALK_MIN_BATCH, ops._walk_partition
    x = d.x.to(dev).requires_grad_(True)
    H = d.H.to(dev).requires_grad_(True)
    c = d.c.to(dev)
    assert L.fl_debug_set_walk(mode, wgs, slices, None) == 0
    try:
        if min_batch is not None:
            ops._WALK_MIN_BATCH = min_batch
        if null_bounds:
            ops._walk_partition = lambda *a: None
        assert ops._walk_applies(nfft, B, NI, NO) and ops._walk_applies(nfft, B, NO, NI)
        ns = int(L.fl_spec_gradh_slices(nfft, B))
        assert ns == min(slices, B)
        _poison(dev, d, ns)          # (behind the inputs: what it hands the allocator is for the operator's own buffers)
        ops.kernel_timer.reset(True)
        y = ops.spectral_apply(x, ops.permute_bins(H, nfft), nfft)
        loss = (y * c).sum() if d.objective == "dot" else ops.mean_square(y)
        gx, gH = torch.autograd.grad(loss, [x, H])
        torch.cuda.synchronize()
        used = {k: len(v) for k, v in ops.kernel_timer.records.items()}
    finally:
        ops.kernel_timer.reset(False)
        ops._WALK_MIN_BATCH, ops._walk_partition = keep
        L.fl_debug_set_walk(1, 0, 0, None)
        ops._GRAD_COLS_SEEN.discard(ops._grad_cols_key(x, nfft, NI, NO))      # (mean_square remembers the shape)
    want = {f"spec_mid_walk[{NI}->{NO},spec]": 1, f"spec_mid_walk[{NO}->{NI}]": 1, "spec_gradh_walk": 1}
    if ns > 1:
        want["sum_parts"] = 1
    rows = {k: v for k, v in used.items() if k.startswith(("spec_mid", "spec_gradh", "sum_parts", "mimo_gradh"))}
    assert rows == want, (rows, want)
    assert used.get("spec_cols_fwd") == 2 and used.get("spec_cols_inv") == 2, used
    return y.detach().cpu(), gx.cpu(), gH.cpu()


# ----------------------------------------------------------------------------- 2. every instantiation
@pytest.mark.gpu
@pytest.mark.parametrize("NO", CHANNELS)
@pytest.mark.parametrize("NI", CHANNELS)
@pytest.mark.parametrize("nfft", [24000, 65536])
def test_every_instantiation(gpu, nfft, NI, NO):
    """The 9 channel pairs at 240- and 256-bin rows, batch 5, the grid of a 256-CU card, one slice: spec_mid_walk<NI, NO> with
    the spectrum kept, spec_mid_walk<NO, NI> as the adjoint (gx), spec_gradh_walk<NI, NO>"""
    d = _data(nfft, NI, NO, 5)
    _check("", _run(gpu, d, CU_256), d)


@pytest.mark.gpu
@pytest.mark.parametrize("NI,NO", [(8, 8), (4, 8), (8, 2)])
@pytest.mark.parametrize("nfft", [60000, 64000])
def test_every_instantiation_odd_columns(gpu, nfft, NI, NO):
    """Odd L1 (125 x 240, 125 x 256): DC / Nyquist is the only self-mirrored row pair"""
    assert PLANS[nfft][0] % 2 == 1
    d = _data(nfft, NI, NO, 5)
    _check("", _run(gpu, d, CU_256), d)


# ----------------------------------------------------------------------------- 3. partitions
@pytest.mark.gpu
@pytest.mark.parametrize("B", [4, 5])
@pytest.mark.parametrize("NI,NO", [(8, 8), (2, 4)])
@pytest.mark.parametrize("nfft", [24000, 65536])
def test_partitions(gpu, nfft, NI, NO, B):
    """One workgroup for everything, 3 (no XCD reordering; whole row pairs inside a range), 8, 16, 40 (empty ranges at 24000)
    and one per unit: float64 per block at one workgroup, bit-identical at every other count"""
    d = _data(nfft, NI, NO, B)
    base = _run(gpu, d, WGS_LADDER[0])
    _check("", base, d)
    for wgs in WGS_LADDER[1:]:
        _same(f"wgs{wgs}_", _run(gpu, d, wgs), base, d)


# ----------------------------------------------------------------------------- 4. null bounds
@pytest.mark.gpu
def test_null_bounds(gpu):
    """bounds == nullptr (ops._walk_partition returns None inside a graph capture with a cold cache): the kernel's own equal-count
    split, bit-identical to the cost-balanced partition's results"""
    d = _data(24000, 8, 8, 5)
    base = _run(gpu, d, 1)
    _check("", base, d)
    for wgs in (3, 16):
        _same(f"wgs{wgs}_", _run(gpu, d, wgs, null_bounds=True), base, d)


# ----------------------------------------------------------------------------- 5. short batches
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("N", [8, 4])
def test_short_batches(gpu, N, B):
    """ops._WALK_MIN_BATCH = 1: the C entries take any batch, so segments of one, two and three units must be right (at one
    item every row pair is fill, one unit, drain; the backward kernel's slice is prologue and epilogue only)"""
    d = _data(24000, N, N, B)
    base = _run(gpu, d, 1, min_batch=1)
    _check("", base, d)
    _same("wgs8_", _run(gpu, d, 8, min_batch=1), base, d)


# ----------------------------------------------------------------------------- 6. batch slices
@pytest.mark.gpu
@pytest.mark.parametrize("B", [4, 5, 7])
@pytest.mark.parametrize("nfft,NI,NO", [(24000, 8, 8), (24000, 4, 4), (24000, 8, 2), (24000, 2, 2), (65536, 8, 8)])
def test_batch_slices(gpu, nfft, NI, NO, B):
    """slices 1, 2, 3 and one per item: slices of one item, of 1 and 2, of 2 and 3 items, up to 7 partial planes through
    fl_sum_parts_c64.  8 -> 8: DEPTH 2, NSC 2; 4 -> 4: DEPTH 1, NSC 2; 8 -> 2 and 2 -> 2: NSC 1.  y and gx do not depend on the
    slices (bit-identical); gH is summed in another order: float64 per row pair"""
    d = _data(nfft, NI, NO, B)
    base = _run(gpu, d, 16, slices=1)
    _check("", base, d)
    for s in (2, 3, B):
        res = _run(gpu, d, 16, slices=s)
        _same(f"s{s}_", res, base, d, only=("y", "gx"))
        _check(f"s{s}_", res, d, only=("gH",))


@pytest.mark.gpu
def test_mode_15(gpu):
    """fl_debug_set_walk(15, ...): spec_gradh_walk<16, 15, 8, 8, NSC = 1, DEPTH 1>, all eight output channels in one workgroup.
    The span name is the same in both modes: what shows that the library took the mode is its own slice count for a full card"""
    L = _lib()
    cus, P = torch.cuda.get_device_properties(gpu).multi_processor_count, PLANS[24000][0] // 2 + 1
    try:            # the slice count that fills the card: CUs / (2 row pairs) with two workgroups per row pair, CUs / row pairs with one
        assert L.fl_debug_set_walk(1, 0, 0, None) == 0 and L.fl_spec_gradh_slices(24000, 1 << 10) == max(cus // (2 * P), 1)
        assert L.fl_debug_set_walk(15, 0, 0, None) == 0 and L.fl_spec_gradh_slices(24000, 1 << 10) == max(cus // P, 1)
    finally:
        L.fl_debug_set_walk(1, 0, 0, None)
    d = _data(24000, 8, 8, 5)
    base = _run(gpu, d, 16, slices=1)
    for s in (1, 2, 5):
        res = _run(gpu, d, 16, slices=s, mode=15)
        _same(f"s{s}_", res, base, d, only=("y", "gx"))
        _check(f"s{s}_", res, d, only=("gH",))


@pytest.mark.gpu
def test_sliced_planes_take_out_scale(gpu):
    """ops.mean_square(y) as the objective: the backward pass runs on y itself and the objective's device factor is multiplied
    into each of the three partial planes (and into gx by its column pass); against the float64 gradient of (y ** 2).mean()"""
    d = _data(24000, 8, 8, 7, objective="mean_square")
    _check("", _run(gpu, d, 16, slices=3), d)


# ----------------------------------------------------------------------------- 7. policy bits
@pytest.mark.gpu
def test_policy_bits(gpu):
    """Bits 4-9 of the stream policy choose other instantiations of the same accesses (non-temporal LDS-DMA, plain stores): the
    results are bit-identical.  Bit 14 walks a slice's items first to last: y and gx bit-identical, gH against float64"""
    L = _lib()
    d = _data(24000, 8, 8, 5)
    mask0 = L.fl_set_stream_policy(0xFFFFFFFF, -1) & 0xFFFFFFFF
    try:
        base = _run(gpu, d, 16, slices=2)
        _check("", base, d)
        for bit in (4, 5, 6, 7, 8, 9):
            assert L.fl_set_stream_policy(mask0 ^ (1 << bit), -1) & 0xFFFFFFFF == mask0 ^ (1 << bit)
            _same(f"bit{bit}_", _run(gpu, d, 16, slices=2), base, d)
        L.fl_set_stream_policy(mask0 ^ (1 << 14), -1)
        res = _run(gpu, d, 16, slices=2)
        _same("bit14_", res, base, d, only=("y", "gx"))
        _check("bit14_", res, d, only=("gH",))
    finally:
        L.fl_set_stream_policy(mask0, -1)
    assert L.fl_set_stream_policy(0xFFFFFFFF, -1) & 0xFFFFFFFF == mask0
