"""The solve routes that take a MATERIALISED per-bin matrix -- fl_solve_*, fl_solve_ws_*, fl_solve_scaled_*, fl_solve_scaled_keep_*
and fl_solve_kept_adjoint_*, through ops.solve and ops.solve_scaled_loop -- on systems that exchange rows, against LAPACK.

Inputs are rounded to the kernel's precision and then held in float64: the reference solves exactly the system the kernel is
given.  Two kinds of system matrix:
  gauss   complex Gaussian entries (ops.solve), or gains of 2..4 on a unit-modulus D times an orthogonal U (the scaled loop): the
          pivot row sits at an arbitrary distance, most steps exchange, condition numbers up to ~1e4
  shift   I - diag(g e^{i phi}) (3 x cyclic shift + 0.05 noise): EVERY elimination step must exchange, condition number 2-3
test_inputs_exchange_rows (host) holds the inputs to that.

Tolerances are LAPACK's own error at the kernel's precision, computed here on the CPU:
  eta      = ||b - A x||_2 / (||A||_F ||x||_2 + ||b||_2)   per (batch item, bin, column), in complex128 on the rounded inputs
  eta_ref  = max eta of torch.linalg.solve on the CPU in complex64 / complex128
  required   max eta of the kernel <= 4 eta_ref   (another elimination order, a hardware reciprocal for the division, threshold
             pivoting in the in-place kernels)
  forward    per bin ||x - x_ref|| <= 2 kappa_f 4 eta_ref ||x_ref|| (forward error <= condition number x backward error, for the
             kernel's solution and the reference's), whole tensor check_close at kappa_max.  kappa_f is torch.linalg.cond in
             the norms eta is written in, ||A||_F ||A^-1||_2 (see _kappa): with the plain 2-norm number the inequality is no
             theorem -- eta divides by ||A||_F, up to sqrt(N) above ||A||_2 -- and the well-conditioned shift systems at
             N = 138 then pass or fail with the host's LAPACK build (eta_ref differed by 0.48x to 1.53x between two hosts)
  gradients  float64 autograd through torch.linalg.solve, check_close at 4 kappa_max 4 eta_ref (two solves feed each product);
             the right-hand side's gradient is an adjoint solve: the eta bound on A^H against LAPACK's on A^H
The achieved errors are recorded under solve_routes/... (tests/golden/achieved_errors.json, conftest.check_close)."""
import functools
import math

import pytest
import torch

from conftest import check_close

M = 67                    # no multiple of any kernel's bins per workgroup (64, 32, 16, 8, 4), several workgroups at every size
C64, C128 = torch.complex64, torch.complex128
KINDS = ("gauss", "shift")
FACTOR = 4.0              # eta_kernel <= FACTOR eta_ref

SOLVE_INPLACE = (2, 3, 4, 5, 8, 9, 13, 16)          # in-place kernels given a P (4, 8, 16 lanes; 16: staged through LDS)
SOLVE_SHUFFLE_32 = (17, 24, 31, 32)
SOLVE_SHUFFLE_64 = (33, 48, 63, 64)                 # complex64 only
SCALED_BOTH = (3, 8, 13, 16, 17, 31, 32)
SCALED_C64 = (33, 63, 64, 65, "max")
SCALED_C128 = (33, "max")
KEPT_BOTH = (3, 4, 5, 13, 16, 17, 31, 32)
KEPT_C64 = (63, 64)
BIG = ("reg+1", "max", "max+1")                     # LDS kernel (fl_solve_*) twice, workspace form (fl_solve_ws_*)


def _sfx(cd):
    return "c64" if cd == C64 else "c128"


def _reg_limit(cd):
    return 64 if cd == C64 else 32


def _max_n(cd):
    from flamo_amd import _lib
    return int(_lib.lib().fl_solve_max_n(int(cd == C128)))


def _size(n, cd):
    """A size given by name, from the library's limits for this precision"""
    if n == "reg+1":
        return _reg_limit(cd) + 1
    if n == "max":
        return _max_n(cd)
    if n == "max+1":
        return _max_n(cd) + 1
    return int(n)


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(k) * 1009 ** i for i, k in enumerate(key)) + 20261020)
    return g


def _round(t, cd):
    return t.to(cd).to(C128)


def _rand(gen, *shape):
    return torch.rand(*shape, dtype=torch.float64, generator=gen)


def _randn(gen, *shape, dtype=torch.float64):
    return torch.randn(*shape, dtype=dtype, generator=gen)


def _shift_mix(gen, N):
    """3 x the cyclic shift + 0.05 noise: the recipe of test_factored_solve_all_sizes_and_row_exchanges"""
    perm = torch.roll(torch.arange(N), 1)
    return 3.0 * torch.eye(N, dtype=torch.float64)[perm] + 0.05 * _randn(gen, N, N)


def _system_matrix(kind, N, m=M):
    """A (m, N, N) complex128, before rounding, for ops.solve"""
    gen = _gen(KINDS.index(kind), N, 1)
    if kind == "gauss":
        return _randn(gen, m, N, N, dtype=C128) / math.sqrt(N)
    g = 0.8 + 0.4 * _rand(gen, N)
    phi = 2 * math.pi * _rand(gen, m, N)
    W = _shift_mix(gen, N).to(C128)
    return torch.eye(N, dtype=C128) - (g * torch.exp(1j * phi)).unsqueeze(-1) * W


def _scaled_factors(kind, N, m=M):
    """g (N,), D (m, N, N), U (N, N) complex128, before rounding, for ops.solve_scaled_loop: A = I - diag(g) D U"""
    gen = _gen(KINDS.index(kind), N, 2)
    if kind == "gauss":
        g = 2.0 + 2.0 * _rand(gen, N)
        D = torch.exp(2j * math.pi * _rand(gen, m, N, N))
        U = torch.linalg.qr(_randn(gen, N, N))[0]
    else:
        D = torch.diag_embed(torch.exp(2j * math.pi * _rand(gen, m, N)))
        U = _shift_mix(gen, N)
        g = 0.8 + 0.4 * _rand(gen, N)
    return g.to(C128), D.to(C128), U.to(C128)


def _scaled_matrix(g, D, U):
    return torch.eye(U.shape[0], dtype=C128) - g.unsqueeze(-1) * (D @ U)


# ---------------------------------------------------------------------------------------------- error measures (CPU, complex128)
def _eta(A, x, b):
    """Normwise backward error of x for A x = b: A (m, N, N), x and b (B, m, N, K) -> (B, m, K)"""
    r = b - torch.einsum("fij,bfjk->bfik", A, x)
    nA = torch.linalg.matrix_norm(A).view(1, -1, 1)
    nx, nb, nr = (torch.linalg.vector_norm(t, dim=2) for t in (x, b, r))
    return nr / (nA * nx + nb)


def _kappa(A):
    """Per bin, the condition number for which forward error <= kappa x eta holds with eta as defined above:
    ||x - y|| = ||A^-1 r|| <= ||A^-1||_2 eta (||A||_F ||y|| + ||b||) <= eta ||A||_F ||A^-1||_2 (||y|| + ||x||), i.e.
    torch.linalg.cond (2-norm) times ||A||_F / ||A||_2"""
    return torch.linalg.cond(A) * torch.linalg.matrix_norm(A) / torch.linalg.matrix_norm(A, ord=2)


def _lapack_eta(A, b, cd):
    """max eta of torch.linalg.solve on the CPU in the kernel's precision"""
    x = torch.linalg.solve(A.to(cd).unsqueeze(0), b.to(cd))
    return _eta(A, x.to(C128), b).max().item()


def _loss(Y, C):
    return torch.sum(torch.real(Y * torch.conj(C)))


class _Report:
    """Every figure of a test is printed before the test fails on any of them"""

    def __init__(self):
        self.bad = []

    def require(self, ok, msg):
        if not ok:
            self.bad.append(msg)

    def close(self, name, got, ref, tol):
        try:
            check_close(name, got, ref, tol, max_tol=float("inf"))
        except AssertionError as e:
            self.bad.append(str(e))

    def solution(self, name, A, x, b, eta_ref, x_ref, kappa, record=True):
        """x solves A x = b: backward error within FACTOR of LAPACK's, forward error per bin and (recorded) over the whole tensor"""
        eta = _eta(A, x, b).max().item()
        print(f"[eta] {name}: kernel {eta:.3e}  lapack {eta_ref:.3e}  ratio {eta / eta_ref:.2f}")
        self.require(eta <= FACTOR * eta_ref, f"{name}: backward error {eta:.3e} is {eta / eta_ref:.2f} x LAPACK's {eta_ref:.3e}")
        err = torch.linalg.vector_norm((x - x_ref).transpose(0, 1).flatten(1), dim=1)
        lim = 2 * kappa * FACTOR * eta_ref * torch.linalg.vector_norm(x_ref.transpose(0, 1).flatten(1), dim=1)
        worst = (err / lim).max().item()
        print(f"[fwd] {name}: largest per-bin forward error / bound {worst:.3f}")
        self.require(worst <= 1.0, f"{name}: per-bin forward error is {worst:.3f} x its bound 2 kappa_f 4 eta_ref")
        if record:
            self.close(name, x, x_ref, 2 * kappa.max().item() * FACTOR * eta_ref)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


# ---------------------------------------------------------------------------------------------- references (CPU, computed once)
@functools.lru_cache(maxsize=None)
def _solve_case(kind, N, cd, one_minus, B=2, K=3, m=M):
    """ops.solve: inputs rounded to cd, held in complex128; LAPACK's solution, gradients, condition numbers and backward errors"""
    A0 = _system_matrix(kind, N, m)
    eye = torch.eye(N, dtype=C128)
    P = _round(eye - A0 if one_minus else A0, cd)
    gen = _gen(KINDS.index(kind), N, 3)
    R = _round(_randn(gen, B, m, N, K, dtype=C128), cd)
    C = _round(_randn(gen, B, m, N, K, dtype=C128), cd)
    Pr, Rr = P.clone().requires_grad_(True), R.clone().requires_grad_(True)
    Y = torch.linalg.solve((eye - Pr if one_minus else Pr).unsqueeze(0), Rr)
    gP, gR = torch.autograd.grad(_loss(Y, C), [Pr, Rr])
    A = eye - P if one_minus else P
    return dict(P=P, R=R, C=C, A=A, Y=Y.detach(), g_P=gP, g_R=gR, kappa=_kappa(A),
                eta_ref=_lapack_eta(A, R, cd), eta_ref_adj=_lapack_eta(A.mH, C, cd))


@functools.lru_cache(maxsize=None)
def _scaled_case(kind, N, cd, B=2, K=3):
    """ops.solve_scaled_loop: the same for A = I - diag(g) D U"""
    g, D, U = (_round(t, cd) for t in _scaled_factors(kind, N))
    gen = _gen(KINDS.index(kind), N, 4)
    R = _round(_randn(gen, B, M, N, K, dtype=C128), cd)
    C = _round(_randn(gen, B, M, N, K, dtype=C128), cd)
    gr, Ur, Rr = (t.clone().requires_grad_(True) for t in (g, U, R))
    Y = torch.linalg.solve(_scaled_matrix(gr, D, Ur).unsqueeze(0), Rr)
    g_g, g_U, g_R = torch.autograd.grad(_loss(Y, C), [gr, Ur, Rr])
    A = _scaled_matrix(g, D, U)
    return dict(g=g, D=D, U=U, R=R, C=C, A=A, Y=Y.detach(), g_g=g_g, g_U=g_U, g_R=g_R, kappa=_kappa(A),
                eta_ref=_lapack_eta(A, R, cd), eta_ref_adj=_lapack_eta(A.mH, C, cd))


# ---------------------------------------------------------------------------------------------- host: the inputs do what they are for
def _lapack_exchanges(A):
    """(m, N - 1) bool: LAPACK's partial pivoting exchanges rows at step k of bin f"""
    N = A.shape[-1]
    piv = torch.linalg.lu_factor(A)[1]
    return piv[:, :N - 1] != torch.arange(1, N, dtype=piv.dtype)


def _threshold_exchanges(A):
    """The same for the in-place kernels' rule (csrc/solve.hip, solve_inplace_kernel): the diagonal stays when its |re| + |im| is
    within a factor 2 of the column's maximum at or below it, else the row of that maximum comes up.  Plain elimination, the bins
    side by side."""
    A = A.clone()
    m, N, _ = A.shape
    rows = torch.arange(m)
    ex = torch.zeros(m, N - 1, dtype=torch.bool)
    for k in range(N - 1):
        mag = A[:, k:, k].real.abs() + A[:, k:, k].imag.abs()
        top, at = mag.max(dim=1)
        ex[:, k] = 2 * mag[:, 0] < top
        p = torch.where(ex[:, k], at + k, torch.full_like(at, k))
        rk, rp = A[rows, k].clone(), A[rows, p].clone()
        A[rows, k], A[rows, p] = rp, rk
        mult = A[:, k + 1:, k] / A[:, k, k].unsqueeze(-1)
        A[:, k + 1:, k + 1:] -= mult.unsqueeze(-1) * A[:, k, k + 1:].unsqueeze(1)
    return ex


def _gpu_matrices():
    """(label, kind, N, A in complex128 after rounding) of every system the GPU tests below solve"""
    for cd in (C64, C128):
        big = [_size(n, cd) for n in BIG]
        sizes = SOLVE_INPLACE + SOLVE_SHUFFLE_32 + (SOLVE_SHUFFLE_64 if cd == C64 else ()) + tuple(big)
        eye = lambda N: torch.eye(N, dtype=C128)      # noqa: E731
        for kind in KINDS:
            for N in sizes:
                A0 = _system_matrix(kind, N)
                yield f"solve/{kind}_N{N}_{_sfx(cd)}_P", kind, N, _round(A0, cd)
                yield f"solve/{kind}_N{N}_{_sfx(cd)}_I-P", kind, N, eye(N) - _round(eye(N) - A0, cd)
            named = (SCALED_C64 + KEPT_C64) if cd == C64 else SCALED_C128
            for N in sorted({_size(n, cd) for n in SCALED_BOTH + KEPT_BOTH + named}):
                g, D, U = (_round(t, cd) for t in _scaled_factors(kind, N))
                yield f"scaled/{kind}_N{N}_{_sfx(cd)}", kind, N, _scaled_matrix(g, D, U)


def test_inputs_exchange_rows():
    """Conditions on the inputs, in float64 on the CPU (a seed that misses one is changed, not the condition).  shift: LAPACK
    exchanges rows at every step 0..N-2 of every bin and so does the in-place kernels' threshold rule; condition number < 10.
    gauss, N >= 5: at least half of all (bin, step) pairs exchange under LAPACK; condition number < 1e5."""
    seen = 0
    for label, kind, N, A in _gpu_matrices():
        ex = _lapack_exchanges(A)
        kappa = torch.linalg.cond(A).max().item()
        if kind == "shift":
            thr = _threshold_exchanges(A)
            assert bool(ex.all()), (label, "LAPACK keeps a diagonal", int(ex.sum()), ex.numel())
            assert bool(thr.all()), (label, "the threshold rule keeps a diagonal", int(thr.sum()), thr.numel())
            assert kappa < 10, (label, kappa)
        else:
            if N >= 5:
                assert 2 * int(ex.sum()) >= ex.numel(), (label, int(ex.sum()), ex.numel())
            assert kappa < 1e5, (label, kappa)
        seen += 1
    assert seen > 150


# ---------------------------------------------------------------------------------------------- (a), (b) ops.solve
def _run_solve(gpu, rep, N, cd, variant=0, B=2, K=3, kinds=KINDS, tag="solve"):
    """ops.solve forward and backward for both kinds and both one_minus values at one size, under one kernel variant"""
    from flamo_amd import _lib, ops
    name_v = "_shfl" if variant == 1 else ""
    for kind in kinds:
        for one_minus in (False, True):
            c = _solve_case(kind, N, cd, one_minus, B, K)
            Pd = c["P"].to(gpu, cd).requires_grad_(True)
            Rd = c["R"].to(gpu, cd).requires_grad_(True)
            _lib.lib().fl_debug_set_solve_variant(variant)
            try:
                Y = ops.solve(Pd, Rd, one_minus=one_minus)
                gP, gR = torch.autograd.grad(_loss(Y, c["C"].to(gpu, cd)), [Pd, Rd])
                torch.cuda.synchronize()
            finally:
                _lib.lib().fl_debug_set_solve_variant(0)
            name = f"solve_routes/{tag}/{kind}_N{N}_{_sfx(cd)}_om{int(one_minus)}{name_v}"
            Y, gP, gR = (t.detach().cpu().to(C128) for t in (Y, gP, gR))
            rep.solution(name + "/Y", c["A"], Y, c["R"], c["eta_ref"], c["Y"], c["kappa"])
            rep.solution(name + "/g_R", c["A"].mH, gR, c["C"], c["eta_ref_adj"], c["g_R"], c["kappa"], record=False)
            rep.close(name + "/g_P", gP, c["g_P"], 4 * c["kappa"].max().item() * FACTOR * c["eta_ref"])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("N", SOLVE_INPLACE)
def test_solve_in_place_sizes(gpu, N, variant):
    """(a) fl_solve_* at N <= 16: the in-place kernels given a P (4, 8 and 16 lanes per bin; 16 lanes load through LDS in chunks
    of four rows, partial at N = 9 and 13), and the shuffle kernel forced at the same sizes (variant 1)"""
    rep = _Report()
    for cd in (C64, C128):
        _run_solve(gpu, rep, N, cd, variant)
    rep.done()


@pytest.mark.gpu
@pytest.mark.parametrize("N", SOLVE_SHUFFLE_32 + SOLVE_SHUFFLE_64)
def test_solve_shuffle_sizes(gpu, N):
    """(a) fl_solve_* at 16 < N <= 64: the shuffle kernel with 32 lanes per bin, and 64 (complex64 only)"""
    rep = _Report()
    for cd in (C64, C128):
        if N <= _reg_limit(cd):
            _run_solve(gpu, rep, N, cd)
    rep.done()


@pytest.mark.gpu
@pytest.mark.parametrize("cd", [C64, C128], ids=_sfx)
@pytest.mark.parametrize("where", BIG)
def test_solve_lds_and_workspace_sizes(gpu, where, cd):
    """(b) beyond the register-resident sizes: the LDS kernel just above the register limit and at fl_solve_max_n, the workspace
    form one above it; 21 right-hand-side columns (several column blocks of the kernel, the last one ragged)"""
    from flamo_amd import _lib
    N = _size(where, cd)
    assert (_lib.lib().fl_solve_ws_bytes(N, M, int(cd == C128)) > 0) == (where == "max+1")
    rep = _Report()
    _run_solve(gpu, rep, N, cd, B=3, K=7, tag="big")
    rep.done()


@pytest.mark.gpu
def test_solve_workspace_bin_walk(gpu):
    """(b) the workspace form with more bins than workspace slots: a workgroup walks f, f + gridDim.x, ... and factors each of its
    bins in the same slot.  Forward only, one right-hand side, complex64, every step an exchange."""
    from flamo_amd import _lib, ops
    L = _lib.lib()
    N = _max_n(C64) + 1
    slots = L.fl_solve_ws_bytes(N, 1 << 20, 0) // (N * (N + 1) * 8)
    m = slots + 3
    assert 0 < slots < m and L.fl_solve_ws_bytes(N, m, 0) == slots * N * (N + 1) * 8
    A = _round(_system_matrix("shift", N, m), C64)
    assert bool(_lapack_exchanges(A).all())
    R = _round(_randn(_gen(N, m), 1, m, N, 1, dtype=C128), C64)
    x_ref = torch.linalg.solve(A.unsqueeze(0), R)
    Y = ops.solve(A.to(gpu, C64), R.to(gpu, C64), one_minus=False)
    torch.cuda.synchronize()
    rep = _Report()
    rep.solution(f"solve_routes/big/walk_shift_N{N}_c64/Y", A, Y.cpu().to(C128), R, _lapack_eta(A, R, C64), x_ref, _kappa(A))
    rep.done()


# ---------------------------------------------------------------------------------------------- (c) ops.solve_scaled_loop
def _scaled_sizes():
    out = [(n, C64) for n in SCALED_BOTH + SCALED_C64] + [(n, C128) for n in SCALED_BOTH + SCALED_C128]
    return [pytest.param(n, cd, id=f"{n}-{_sfx(cd)}") for n, cd in out]


@pytest.mark.gpu
@pytest.mark.parametrize("n,cd", _scaled_sizes())
def test_scaled_loop_sizes(gpu, n, cd):
    """(c) (I - diag(g) D U)^-1 R through fl_solve_scaled_* at every kernel shape up to fl_solve_max_n -- above 64 (complex64) /
    32 (complex128) the LDS kernel applies the gains where it loads the matrix -- with the gradients of g, U and R, the adjoint
    system from kept factors (ops.KEEP_LU, 16 < N <= 64 / 32) and from a second elimination"""
    from flamo_amd import ops
    N = _size(n, cd)
    rep = _Report()
    for kind in KINDS:
        c = _scaled_case(kind, N, cd)
        for keep in (True, False):
            gd, Ud, Rd = (c[k].to(gpu, cd).requires_grad_(True) for k in ("g", "U", "R"))
            ops.KEEP_LU = keep
            try:
                Y = ops.solve_scaled_loop(gd, c["D"].to(gpu, cd), Ud, Rd)
                got = torch.autograd.grad(_loss(Y, c["C"].to(gpu, cd)), [gd, Ud, Rd])
                torch.cuda.synchronize()
            finally:
                ops.KEEP_LU = True
            Y, g_g, g_U, g_R = (t.detach().cpu().to(C128) for t in (Y, *got))
            name = f"solve_routes/scaled/{kind}_N{N}_{_sfx(cd)}_keep{int(keep)}"
            rep.solution(name + "/Y", c["A"], Y, c["R"], c["eta_ref"], c["Y"], c["kappa"])
            rep.solution(name + "/g_R", c["A"].mH, g_R, c["C"], c["eta_ref_adj"], c["g_R"], c["kappa"], record=False)
            tol = 4 * c["kappa"].max().item() * FACTOR * c["eta_ref"]
            rep.close(name + "/g_g", g_g, c["g_g"], tol)
            rep.close(name + "/g_U", g_U, c["g_U"], tol)
    rep.done()


# ---------------------------------------------------------------------------------------------- (d) kept factors, called directly
@pytest.mark.gpu
@pytest.mark.parametrize("N", KEPT_BOTH + KEPT_C64)
def test_kept_factors_every_size(gpu, N):
    """(d) fl_solve_scaled_keep_* and fl_solve_kept_adjoint_* at sizes the op does not send them (N <= 16) and at odd N, where
    the float kernel stores its factors element by element: the forward solution, the adjoint solution from the kept factors,
    and the forward solution bit-equal to fl_solve_scaled_* on the same (shuffle) kernel.  The kept arrays stay opaque."""
    from flamo_amd import _lib, ops
    rep = _Report()
    for cd in (C64, C128):
        if N > _reg_limit(cd):
            continue
        for kind in KINDS:
            c = _scaled_case(kind, N, cd)
            # planar operands as _SolveScaledLoop.forward prepares them
            Dp = ops._h_planar(c["D"].to(gpu, cd), True)
            gc, Uc = c["g"].to(gpu, cd).contiguous(), c["U"].to(gpu, cd).contiguous()
            Rp, Cp = ops.to_planar(c["R"].to(gpu, cd)), ops.to_planar(c["C"].to(gpu, cd))
            DU = ops._mimo_launch(Uc.transpose(-1, -2), False, False, False, ops.to_planar(Dp.permute(1, 0, 2))).permute(1, 0, 2)
            OUT, LU, piv = ops._solve_scaled_launch(DU, gc, False, Rp, keep=True)
            ADJ = ops._solve_kept_adjoint_launch(LU, piv, Cp)
            _lib.lib().fl_debug_set_solve_variant(1 if N <= 16 else 0)
            try:
                PLAIN = ops._solve_scaled_launch(DU, gc, False, Rp)
                torch.cuda.synchronize()
            finally:
                _lib.lib().fl_debug_set_solve_variant(0)
            name = f"solve_routes/kept/{kind}_N{N}_{_sfx(cd)}"
            rep.solution(name + "/OUT", c["A"], OUT.cpu().to(C128), c["R"], c["eta_ref"], c["Y"], c["kappa"])
            rep.solution(name + "/ADJ", c["A"].mH, ADJ.cpu().to(C128), c["C"], c["eta_ref_adj"], c["g_R"], c["kappa"], record=False)
            rep.require(torch.equal(OUT, PLAIN), f"{name}: the forward solution differs from fl_solve_scaled's on the same kernel")
    rep.done()


# ---------------------------------------------------------------------------------------------- (e) refusals
@pytest.mark.gpu
@pytest.mark.parametrize("cd", [C64, C128], ids=_sfx)
def test_scaled_loop_refuses_beyond_max_n(gpu, cd):
    """(e) fl_solve_scaled_* has no workspace form: one above fl_solve_max_n the op raises with the library's message"""
    from flamo_amd import ops
    N, m = _max_n(cd) + 1, 5
    g, D, U = (t.to(gpu, cd) for t in _scaled_factors("shift", N, m))
    R = torch.ones(1, m, N, 1, dtype=cd, device=gpu)
    with pytest.raises(RuntimeError, match=rf"solve_scaled: N={N} exceeds fl_solve_max_n \({N - 1} for this precision\)"):
        ops.solve_scaled_loop(g, D, U, R)
    torch.cuda.synchronize()
