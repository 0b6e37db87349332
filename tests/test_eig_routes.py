"""The per-bin eigenvalue kernel (csrc/eig.hip: ops.eigvals, functional.get_eigenvalues) against LAPACK's own backward error.

Inputs are rounded to the kernel's precision and then held in complex128: the reference works on exactly the matrix the kernel
is given.  Every measure is computed in complex128 on the CPU, on the matrix and the spectrum scaled by one power of two per
bin (exact), so that none of them overflows at the outer exponents of `scaled`:
  eta(lambda) = sigma_min(A - lambda I) / ||A||_F   the exact normwise backward error of ONE computed eigenvalue
  tr1         = |sum lambda - tr A| / ||A||_F
  tr2         = |sum lambda^2 - tr A^2| / ||A||_F^2  tr1 and tr2 see a spectrum that returns one eigenvalue twice and misses
                                                     another, which eta cannot
  reference   per measure, the maximum over the bins for torch.linalg.eigvals on the CPU in complex64 / complex128; where
              that is below N eps of the precision (`graded` reaches 1e-20: a few entries dominate ||A||_F; the defective
              families are exact), N eps
  required    kernel <= 4 x reference (FACTOR of test_solve_routes.py, for the same reasons: another elimination order,
              other rotations), and eigvals_info() all zero, for every family at every size
  matched     the families with simple, well separated eigenvalues (gauss, loop, real, herm, scaled): one-to-one greedy
              matching (the closest remaining pair first) against the complex128 LAPACK spectrum, distances over ||A||_F.
              complex64: at most 4 x the matched distance of the complex64 LAPACK spectrum (no floor: it is never
              near zero on these families, test_lapack_stays_inside_every_cap holds it above eps / 4).
              complex128: per eigenvalue at most 2 kappa_lambda 4 eta_ref, kappa_lambda = ||w_i|| ||v_i|| / |w_i^H v_i| from
              torch.linalg.eig on the CPU with W = V^-H (forward error <= condition number x backward error, once for the
              kernel's eigenvalue and once for the reference's).
              jordan_lower and nil_lower are defective -- an eigenvalue of multiplicity N moves by eta^(1/N) -- and
              near_hessenberg, near_triangular, unitary_shift and graded promise no separation: eta, tr1, tr2 and info only.
  gradients   the loss of test_eigvals_kernel_matches_lapack, against complex128 autograd through torch.linalg.eigvals on the
              CPU, families gauss, loop, herm.  complex64: l2 and max-norm error at most 4 x those of the same autograd run in
              complex64 on the CPU.  complex128 has no wider reference to take a figure from: its limit is the complex64 limit
              of the same family and size times 2^-29, the ratio of the unit roundoffs.
The achieved figures are recorded under eig_routes/<family>_<N>_<c64|c128>/... (tests/golden/achieved_errors.json): /ratios holds
1 + measure / reference against 1 for the three measures side by side (its max is the worst ratio, its limit FACTOR; none for
the defective families, where the kernel is exact and a recorded 0 would bind the CPU's SVD, not the kernel), /lam the matched
spectrum, /g_A the gradient.

Families (M = 23 bins, no multiple of anything; G complex Gaussian / sqrt(N)):
  gauss            G
  near_hessenberg  triu(G, -1) + delta tril(G, -2), delta = 1e-9 | 1e-12 (complex128), 1e-5 | 1e-6 (complex64) by bin parity:
                   below sqrt(eps) of the subdiagonal, where a squared norm minus the squared subdiagonal cancels to zero
  near_triangular  triu(G) + delta tril(G, -1), the same deltas
  unitary_shift    phase x the cyclic shift P, phase 1, i, -i, e^{0.3 i}, 0.9 i by bin; N >= 3.  A purely imaginary
                   subdiagonal: Wilkinson shift 0, and an exceptional shift taken from real parts is 0 as well
  loop             diag(0.97 e^{i phi}) U, U orthogonal from a QR: the use case
  real             real Gaussian / sqrt(N) through functional.get_eigenvalues (the real -> complex cast): conjugate pairs
  herm             G + G^H
  graded           diag(10^-linspace(0, 6, N)) G diag(10^linspace(0, 3, N))
  jordan_lower     0.5 I + the LOWER shift (an upper one is already triangular)
  nil_lower        the lower shift alone
  scaled           G 2^k, k = 20, -20, 60, -60 (complex64) / 300, -300, 480, -480 (complex128) by bin
"""
import ctypes
import functools
import math

import pytest
import torch

from conftest import check_close, maxerr, relerr

M = 23
C64, C128 = torch.complex64, torch.complex128
FACTOR = 4.0              # kernel <= FACTOR x LAPACK
FAMILIES = ("gauss", "near_hessenberg", "near_triangular", "unitary_shift", "loop", "real", "herm", "graded", "jordan_lower",
            "nil_lower", "scaled")
MATCHED = ("gauss", "loop", "real", "herm", "scaled")
GRAD_FAMILIES = ("gauss", "loop", "herm")
DEFECTIVE = ("jordan_lower", "nil_lower")
SIZES = (2, 3, 5, 8, 16, 17, 32, 33)
BIG = {C64: (48, 64), C128: (40, 64)}                   # forward only: dynamic LDS above 64 KB
DELTAS = {C64: (1e-5, 1e-6), C128: (1e-9, 1e-12)}
EXPONENTS = {C64: (20, -20, 60, -60), C128: (300, -300, 480, -480)}
PHASES = (1.0 + 0j, 1j, -1j, complex(math.cos(0.3), math.sin(0.3)), 0.9j)
IMAGINARY = (1, 2, 4)     # the entries of PHASES with a purely imaginary subdiagonal
GRAD_BOTH = (3, 8, 17, 32)
LDS_LIMIT = 160 * 1024


def _sfx(cd):
    return "c64" if cd == C64 else "c128"


def _eps(cd):
    return torch.finfo(torch.float32 if cd == C64 else torch.float64).eps


def _rdtype(cd):
    return torch.float32 if cd == C64 else torch.float64


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(k) * 1009 ** i for i, k in enumerate(key)) + 20261021)
    return g


def _round(t, cd):
    return t.to(C128).to(cd).to(C128)


def _pow2(e):
    """2^e exactly, e an integer tensor"""
    return torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e.to(torch.int32))


@functools.lru_cache(maxsize=None)
def _family(family, N, cd, m=M):
    """(m, N, N) complex128 holding values of the precision cd"""
    gen = _gen(FAMILIES.index(family), N)
    G = torch.randn(m, N, N, dtype=C128, generator=gen) / math.sqrt(N)
    eye = torch.eye(N, dtype=C128)
    lower = torch.diag(torch.ones(N - 1, dtype=C128), -1)
    f = torch.arange(m)
    if family == "gauss":
        A = G
    elif family in ("near_hessenberg", "near_triangular"):
        band = -1 if family == "near_hessenberg" else 0
        delta = torch.tensor(DELTAS[cd], dtype=torch.float64)[f % 2].view(m, 1, 1)
        A = torch.triu(G, band) + delta * torch.tril(G, band - 1)
    elif family == "unitary_shift":
        P = eye[torch.roll(torch.arange(N), 1)]                       # P e_k = e_{k+1 mod N}: subdiagonal and the corner
        A = torch.tensor(PHASES, dtype=C128)[f % len(PHASES)].view(m, 1, 1) * P
    elif family == "loop":
        U = torch.linalg.qr(torch.randn(N, N, dtype=torch.float64, generator=gen))[0].to(C128)
        phi = 2 * math.pi * torch.rand(m, N, dtype=torch.float64, generator=gen)
        A = (0.97 * torch.exp(1j * phi)).unsqueeze(-1) * U
    elif family == "real":
        A = (torch.randn(m, N, N, dtype=torch.float64, generator=gen) / math.sqrt(N)).to(C128)
    elif family == "herm":
        A = G + G.mH
    elif family == "graded":
        dl = torch.pow(10.0, -torch.linspace(0, 6, N, dtype=torch.float64)).to(C128)
        dr = torch.pow(10.0, torch.linspace(0, 3, N, dtype=torch.float64)).to(C128)
        A = dl.view(1, N, 1) * G * dr.view(1, 1, N)
    elif family == "jordan_lower":
        A = (0.5 * eye + lower).expand(m, N, N)
    elif family == "nil_lower":
        A = lower.expand(m, N, N)
    elif family == "scaled":
        k = torch.tensor(EXPONENTS[cd])[f % 4]
        return _round(G, cd) * _pow2(k).view(m, 1, 1)                 # exact in cd: 2^60 and 2^480 are far inside its range
    else:
        raise KeyError(family)
    return _round(A.contiguous(), cd)


def _families(N):
    return tuple(fam for fam in FAMILIES if not (fam == "unitary_shift" and N < 3))


# ---------------------------------------------------------------------------------------------- error measures (CPU, complex128)
def _normalised(A, lam):
    """A and lam times the power of two that brings the largest |entry| of each bin to [1, 2): exact, the measures are scale-free"""
    amax = A.abs().amax(dim=(-2, -1))
    e = torch.where(amax > 0, torch.floor(torch.log2(amax.clamp_min(1e-300))), torch.zeros_like(amax))
    s = _pow2(-e)
    return A * s.view(-1, 1, 1), lam * s.view(-1, 1)


def _measures(A, lam):
    """eta (m, N), tr1 (m,), tr2 (m,) of the spectra lam (m, N) of A (m, N, N); a non-finite eigenvalue counts as infinite error"""
    A, lam = _normalised(A, lam)
    N = A.shape[-1]
    finite = torch.isfinite(lam.real) & torch.isfinite(lam.imag)
    lam = torch.where(finite, lam, torch.zeros_like(lam))
    nA = torch.linalg.matrix_norm(A)
    shifted = A.unsqueeze(1) - lam.view(-1, N, 1, 1) * torch.eye(N, dtype=C128)
    inf = torch.full((), float("inf"), dtype=torch.float64)
    eta = torch.where(finite, torch.linalg.svdvals(shifted)[..., -1] / nA.unsqueeze(-1), inf)
    tr1 = (lam.sum(-1) - torch.diagonal(A, dim1=-2, dim2=-1).sum(-1)).abs() / nA
    tr2 = ((lam * lam).sum(-1) - torch.diagonal(A @ A, dim1=-2, dim2=-1).sum(-1)).abs() / nA ** 2
    ok = finite.all(-1)
    return eta, torch.where(ok, tr1, inf), torch.where(ok, tr2, inf)


def _matched(lam, ref):
    """One-to-one greedy matching of the spectra lam to ref, both (m, N): the closest remaining pair first.  Returns the distances
    (m, N) and lam in the order of ref."""
    m, N = ref.shape
    d = (lam.unsqueeze(-1) - ref.unsqueeze(-2)).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, 1e300), d).clamp_max(1e300)
    rows = torch.arange(m)
    dist = torch.empty(m, N, dtype=torch.float64)
    perm = torch.empty(m, N, dtype=torch.long)
    for _ in range(N):
        at = d.flatten(1).argmin(dim=1)
        i, j = at // N, at % N
        dist[rows, j] = d[rows, i, j]
        perm[rows, j] = i
        d[rows, i, :] = float("inf")
        d[rows, :, j] = float("inf")
    return dist, torch.gather(lam, 1, perm)


@functools.lru_cache(maxsize=None)
def _reference(family, N, cd):
    """LAPACK on the CPU at the kernel's precision: its measures (floored at N eps), its spectrum in complex128 with the
    eigenvalue condition numbers, and for complex64 the matched distance of its own spectrum"""
    A = _family(family, N, cd)
    floor = N * _eps(cd)
    lam = torch.linalg.eigvals(A.to(cd)).to(C128)
    eta, tr1, tr2 = (t.max().item() for t in _measures(A, lam))
    raw = dict(eta=eta, tr1=tr1, tr2=tr2)
    ref = dict(A=A, raw=raw, eta=max(eta, floor), tr1=max(tr1, floor), tr2=max(tr2, floor), floor=floor, lam_lapack=lam)
    if family in MATCHED:
        lam128, V = torch.linalg.eig(A)
        W = torch.linalg.inv(V).mH
        ref["lam128"] = lam128
        ref["kappa"] = torch.linalg.vector_norm(W, dim=-2) * torch.linalg.vector_norm(V, dim=-2) / (W.conj() * V).sum(-2).abs()
        ref["nA"] = torch.linalg.matrix_norm(A)
        if cd == C64:
            dist, own = _matched(lam, lam128)
            raw["dist"] = ref["dist"] = (dist / ref["nA"].unsqueeze(-1)).max().item()      # no floor: LAPACK's own figure
            ref["lam_l2"], ref["lam_max"] = relerr(own, lam128), maxerr(own, lam128)
    return ref


class _Report:
    """Every figure of a test is printed before the test fails on any of them"""

    def __init__(self):
        self.bad = []

    def require(self, ok, msg):
        if not ok:
            self.bad.append(msg)

    def close(self, name, got, ref, tol, max_tol=float("inf")):
        try:
            check_close(name, got, ref, tol, max_tol=max_tol)
        except AssertionError as e:
            self.bad.append(str(e))

    def spectrum(self, name, family, N, cd, lam, info):
        """The whole rule for one family at one size: lam (m, N) complex128 from the kernel, info its flags"""
        ref = _reference(family, N, cd)
        A = ref["A"]
        self.require(info == 0, f"{name}: eigvals_info() reports {info}")
        got = dict(zip(("eta", "tr1", "tr2"), _measures(A, lam)))
        ratios = []
        for key, val in got.items():
            worst = val.max().item()
            print(f"[{key}] {name}: kernel {worst:.3e}  lapack {ref['raw'][key]:.3e}  reference {ref[key]:.3e}  "
                  f"ratio {worst / ref[key]:.2f}")
            self.require(worst <= FACTOR * ref[key], f"{name}: {key} {worst:.3e} is {worst / ref[key]:.2f} x the reference {ref[key]:.3e}")
            ratios.append((val / ref[key]).flatten())
        ratios = torch.cat(ratios).clamp_max(1e30)
        if family not in DEFECTIVE:
            # (no record for the defective families: the kernel is exact on them, and a recorded 0 would hold a later run to
            # the CPU's svdvals returning exactly 0, not 1e-17, for sigma_min of a shift matrix)
            self.close(name + "/ratios", 1.0 + ratios, torch.ones_like(ratios), FACTOR * (1 + 1e-12), max_tol=FACTOR * (1 + 1e-12))
        if family not in MATCHED:
            return
        dist, own = _matched(lam, ref["lam128"])
        rel = dist / ref["nA"].unsqueeze(-1)
        if cd == C64:
            worst = rel.max().item()
            print(f"[dist] {name}: kernel {worst:.3e}  lapack {ref['raw']['dist']:.3e}  ratio {worst / ref['dist']:.2f}")
            self.require(worst <= FACTOR * ref["dist"], f"{name}: matched distance {worst:.3e} is {worst / ref['dist']:.2f} x LAPACK's")
            # the same for the whole tensor: l2 and max-norm error within FACTOR of the complex64 LAPACK spectrum's
            self.close(name + "/lam", own, ref["lam128"], FACTOR * ref["lam_l2"], FACTOR * ref["lam_max"])
        else:
            bound = 2 * ref["kappa"] * FACTOR * ref["eta"]
            worst = (rel / bound).max().item()
            print(f"[dist] {name}: largest matched distance / (2 kappa_lambda 4 eta_ref ||A||_F) {worst:.3f}")
            self.require(worst <= 1.0, f"{name}: matched distance is {worst:.3f} x its bound 2 kappa_lambda 4 eta_ref ||A||_F")
            # the same bound for the whole tensor: every |d_j| <= 2 kappa_max 4 eta_ref ||A_f||_F
            tol = 2 * ref["kappa"].max().item() * FACTOR * ref["eta"] * math.sqrt(N) * torch.linalg.vector_norm(ref["nA"]).item()
            self.close(name + "/lam", own, ref["lam128"], tol / torch.linalg.vector_norm(ref["lam128"]).item())

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _kernel_spectrum(gpu, family, N, cd, A=None):
    """The kernel's eigenvalues of the family (or of A), (m, N) complex128 on the CPU, and the largest |info|"""
    from flamo_amd import functional, ops
    A = _family(family, N, cd) if A is None else A
    with torch.no_grad():
        if family == "real":
            lam = functional.get_eigenvalues(A.real.to(gpu, _rdtype(cd)))
        else:
            lam = ops.eigvals(A.to(gpu, cd))
    assert lam.dtype == cd and lam.shape == A.shape[:-1]
    info = int(ops.eigvals_info().abs().max())
    return lam.cpu().to(C128), info


# ---------------------------------------------------------------------------------------------- the LDS bound, from the library
def _fits(N, vectors, cd):
    """The entry's own answer, on the host and without a launch (an empty batch): does N fit with / without eigenvectors"""
    from flamo_amd import _lib
    L = _lib.lib()
    buf = ctypes.addressof(ctypes.create_string_buffer(16))           # never read: M = 0
    fn = L.fl_eig_c64 if cd == C64 else L.fl_eig_c128
    rc = fn(buf, 0, N, 0, buf, 0, buf if vectors else None, 0, None, None)
    if rc != 0:
        msg = L.fl_last_error().decode("utf-8", "replace")
        assert "does not fit in LDS" in msg, msg
    return rc == 0


def _lds_bytes(N, vectors, cd):
    """eig_impl's `lds` expression (csrc/eig.hip): H, Q (and Y) of N x (N + 1), N sines, N cosines"""
    c = 8 if cd == C64 else 16
    return ((3 if vectors else 2) * N * (N + 1) + N) * c + N * (c // 2)


@functools.lru_cache(maxsize=None)
def _grad_max_n(cd):
    """The largest N <= 64 whose three-matrix layout (eigenvectors, for the backward) the library accepts"""
    return max(n for n in range(1, 65) if _fits(n, True, cd))


def test_lds_bound_between_57_and_58():
    """The 160 KB bound of the three-matrix layout falls between N = 57 and N = 58 in complex128 and above 64 in complex64; the
    two-matrix layout (no gradient) holds N = 64 at both precisions.  The library's answer (an empty batch is refused or
    accepted on the host) and the kernel's `lds` expression written out here agree at every N."""
    for cd in (C64, C128):
        for vectors in (False, True):
            for n in range(1, 65):
                assert _fits(n, vectors, cd) == (_lds_bytes(n, vectors, cd) <= LDS_LIMIT), (cd, vectors, n)
        assert _fits(64, False, cd)
    assert _grad_max_n(C64) == 64
    top = _grad_max_n(C128)
    assert _lds_bytes(top, True, C128) <= LDS_LIMIT < _lds_bytes(top + 1, True, C128)
    assert (top, top + 1) == (57, 58)
    assert _lds_bytes(top, True, C128) > 64 * 1024 and _lds_bytes(64, True, C64) > 64 * 1024 and _lds_bytes(40, True, C128) > 64 * 1024


# ---------------------------------------------------------------------------------------------- host: the inputs do what they are for
def _all_sizes(cd):
    return SIZES + BIG[cd]


def _size_params():
    out = [(n, cd) for cd in (C64, C128) for n in _all_sizes(cd)]
    return [pytest.param(n, cd, id=f"{n}-{_sfx(cd)}") for n, cd in out]


@pytest.mark.parametrize("cd", [C64, C128], ids=_sfx)
def test_inputs_have_their_properties(cd):
    """Conditions on the inputs, in float64 on the CPU (a seed that misses one is changed, not the condition).
    near_hessenberg, N >= 3: in every bin the part of a column below the subdiagonal is smaller than sqrt(eps) times the
    subdiagonal entry -- where nrm2 - |x0|^2 cancels to zero -- in at least half of the columns (a Gaussian subdiagonal entry
    is sometimes small), and non-zero in all of them.  near_triangular: the strict lower triangle is non-zero and below
    sqrt(eps) max |A|.  unitary_shift: upper Hessenberg, unitary up to the 0.9 and the rounding, the subdiagonal purely
    imaginary where claimed.  jordan_lower / nil_lower: lower bidiagonal, not upper triangular.  scaled: in the outer bins the
    squared modulus of a product of two entries (the Wilkinson shift's discriminant) overflows, or underflows to zero, at this
    precision."""
    root = math.sqrt(_eps(cd))
    for N in _all_sizes(cd):
        if N >= 3:
            A = _family("near_hessenberg", N, cd)
            sub = torch.diagonal(A, offset=-1, dim1=-2, dim2=-1)[:, :N - 2].abs()
            tail = torch.linalg.vector_norm(torch.tril(A, -2)[:, :, :N - 2], dim=-2)
            assert bool((tail > 0).all())
            small = tail < root * sub
            assert bool((2 * small.sum(-1) >= N - 2).all()), (N, small.sum(-1).min().item())
            U = _family("unitary_shift", N, cd)
            assert bool((torch.tril(U, -2) == 0).all())
            scale = torch.tensor([abs(p) for p in PHASES], dtype=torch.float64)[torch.arange(M) % len(PHASES)]
            assert ((U.mH @ U) / (scale ** 2).view(M, 1, 1) - torch.eye(N, dtype=C128)).abs().max() < 4 * _eps(cd)
            subd = torch.diagonal(U, offset=-1, dim1=-2, dim2=-1)
            assert bool((subd.abs() > 0.5).all())
            for f in range(M):
                if f % len(PHASES) in IMAGINARY:
                    assert bool((subd[f].real == 0).all()) and U[f, 0, N - 1].real == 0
        T = _family("near_triangular", N, cd)
        low = torch.tril(T, -1)
        assert bool((low.abs()[:, torch.tril(torch.ones(N, N), -1) > 0] > 0).all())
        assert low.abs().amax(dim=(-2, -1)).max() < root * T.abs().amax(dim=(-2, -1)).min()
        for fam, d in (("jordan_lower", 0.5), ("nil_lower", 0.0)):
            J = _family(fam, N, cd)
            assert torch.equal(J[0], d * torch.eye(N, dtype=C128) + torch.diag(torch.ones(N - 1, dtype=C128), -1))
            assert bool((J == J[0]).all())
        S = _family("scaled", N, cd).abs().amax(dim=(-2, -1))
        big, small = torch.finfo(_rdtype(cd)).max, torch.finfo(_rdtype(cd)).tiny
        for f in range(M):
            k = EXPONENTS[cd][f % 4]
            assert 2.0 ** (k - 4) < S[f] < 2.0 ** (k + 3)
            if abs(k) in (60, 480):
                assert (S[f] ** 4 > big) if k > 0 else (S[f] ** 4 < small * _eps(cd))
        R = _family("real", N, cd)
        assert bool((R.imag == 0).all())
        H = _family("herm", N, cd)
        assert torch.equal(H, H.mH)


@pytest.mark.parametrize("N,cd", _size_params())
def test_lapack_stays_inside_every_cap(N, cd):
    """LAPACK at the kernel's precision, every family and size the GPU tests use: finite spectra (torch raises on a LAPACK
    info), reference values finite and non-zero after the N eps floor, the matched families' own distance and condition numbers
    finite.  On the families whose ||A||_F is no larger than their spectrum's (gauss, unitary_shift, loop, real, herm, scaled;
    N >= 3) LAPACK's largest eta lies between eps and 16 eps of the precision (seen: 1.5 to 14.3, the upper end on herm): the
    yardstick is roundoff-sized, neither zero nor loose."""
    lo, hi = _eps(cd), 16 * _eps(cd)
    for fam in _families(N):
        ref = _reference(fam, N, cd)
        assert bool(torch.isfinite(ref["lam_lapack"].abs()).all()), (fam, N)
        for key in ("eta", "tr1", "tr2"):
            assert math.isfinite(ref[key]) and ref[key] >= ref["floor"] > 0, (fam, N, key, ref[key])
            assert ref[key] < 1e3 * ref["floor"], (fam, N, key, ref[key])
        if fam in MATCHED:
            assert bool(torch.isfinite(ref["kappa"]).all()) and ref["kappa"].min() >= 1 - 1e-9, (fam, N)
            if cd == C64:
                assert math.isfinite(ref["dist"]) and ref["dist"] > _eps(cd) / 4, (fam, N, ref["dist"])
                assert ref["lam_l2"] > _eps(cd) / 4 and ref["lam_max"] > _eps(cd) / 4, (fam, N, ref["lam_l2"], ref["lam_max"])
        if fam in ("gauss", "unitary_shift", "loop", "real", "herm", "scaled") and N >= 3:
            assert lo < ref["raw"]["eta"] < hi, (fam, N, ref["raw"]["eta"])


# ---------------------------------------------------------------------------------------------- GPU: every family at every size
@pytest.mark.gpu
@pytest.mark.parametrize("N,cd", _size_params())
def test_families_against_lapack_backward_error(gpu, N, cd):
    """Every family at one size and precision (forward, no eigenvectors): eta, tr1, tr2 within 4 x LAPACK's, info zero, and the
    matched distance for the families with separated eigenvalues.  N = 48 / 64 (complex64) and 40 / 64 (complex128) take more
    than 64 KB of dynamic LDS."""
    rep = _Report()
    for fam in _families(N):
        lam, info = _kernel_spectrum(gpu, fam, N, cd)
        rep.spectrum(f"eig_routes/{fam}_{N}_{_sfx(cd)}", fam, N, cd, lam, info)
    rep.done()


# ---------------------------------------------------------------------------------------------- GPU: shapes and views
@pytest.mark.gpu
@pytest.mark.parametrize("cd", [C64, C128], ids=_sfx)
def test_single_matrix_and_leading_dimensions(gpu, cd):
    """Mt = 1 (one workgroup, with and without a leading dimension) and leading dimensions (2, 5): the bits of the same matrices
    in the flat batch, whose spectra the rule above holds"""
    from flamo_amd import ops
    N = 17
    A = _family("gauss", N, cd)
    Ad = A.to(gpu, cd)
    with torch.no_grad():
        flat = ops.eigvals(Ad)
        info_flat = int(ops.eigvals_info().abs().max())
        one = ops.eigvals(Ad[4:5])
        info_one = int(ops.eigvals_info().abs().max())
        bare = ops.eigvals(Ad[4])
        lead = ops.eigvals(Ad[3:13].reshape(2, 5, N, N))
        info_lead = ops.eigvals_info()
    assert one.shape == (1, N) and bare.shape == (N,) and lead.shape == (2, 5, N) and info_lead.shape == (10,)
    assert info_one == 0 and int(info_lead.abs().max()) == 0
    assert torch.equal(one[0], flat[4]) and torch.equal(bare, flat[4]) and torch.equal(lead.reshape(10, N), flat[3:13])
    rep = _Report()
    rep.spectrum(f"eig_routes/shapes_{N}_{_sfx(cd)}", "gauss", N, cd, flat.cpu().to(C128), info_flat)
    rep.done()


@pytest.mark.gpu
@pytest.mark.parametrize("cd", [C64, C128], ids=_sfx)
def test_transposed_and_conjugated_views(gpu, cd):
    """An .mT view and a .conj() view (lazy conjugation) give the bits of the same values made contiguous, forward and backward"""
    from flamo_amd import ops
    N = 8
    Ad = _family("gauss", N, cd).to(gpu, cd)
    for view in (Ad.mT, Ad.conj(), Ad.mH):
        assert not view.is_contiguous() or view.is_conj()
        plain = view.resolve_conj().contiguous()
        assert not plain.is_conj() and plain.is_contiguous() and torch.equal(plain, view)
        out = []
        for x in (view, plain):
            x = x.detach().requires_grad_(True)
            lam = ops.eigvals(x)
            (g,) = torch.autograd.grad(_loss(lam), [x])
            assert int(ops.eigvals_info().abs().max()) == 0
            out.append((lam.detach(), g))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("cd", [C64, C128], ids=_sfx)
def test_info_flags_non_finite_and_only_those_bins(gpu, cd):
    """What a caller gets when a bin cannot be solved: a NaN or an infinite entry sets that bin's flag (the iteration ends at
    its sweep cap or the load notices), its values are unspecified, and the bins beside it -- an all-zero matrix, which keeps
    scale 1, among them -- are flagged 0 and have the bits of a batch without the bad bins"""
    from flamo_amd import ops
    N = 5
    A = _family("gauss", N, cd)[:6].clone()
    A[1, 0, 1] = complex(float("nan"), 0.0)
    A[3, 4, 4] = complex(0.0, float("inf"))
    A[4] = 0
    good = [0, 2, 4, 5]
    with torch.no_grad():
        lam = ops.eigvals(A.to(gpu, cd))
        info = ops.eigvals_info().cpu()
        ref = ops.eigvals(A[good].to(gpu, cd))
        assert int(ops.eigvals_info().abs().max()) == 0
    assert info.dtype == torch.int32 and info.shape == (6,)
    assert bool((info[[1, 3]] > 0).all()) and bool((info[[1, 3]] <= N).all()) and bool((info[good] == 0).all()), info
    assert torch.equal(lam[good], ref) and bool((lam[4] == 0).all())


# ---------------------------------------------------------------------------------------------- gradients
def _loss(lam):
    return ((lam.abs() - 0.7) ** 2).sum() + (lam.real ** 3).sum() * 0.1


def _cpu_grad(A):
    A = A.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(_loss(torch.linalg.eigvals(A)), [A])
    return g


@functools.lru_cache(maxsize=None)
def _grad_case(family, N):
    """complex128 autograd on the CPU of the loss at the complex64-rounded and at the unrounded input, and the error of the same
    autograd run in complex64: the yardstick of both precisions"""
    A64, A128 = _family(family, N, C64), _family(family, N, C128)
    g64_exact, g128 = _cpu_grad(A64), _cpu_grad(A128)
    g64 = _cpu_grad(A64.to(C64)).to(C128)
    return dict(ref={C64: g64_exact, C128: g128}, l2=relerr(g64, g64_exact), max=maxerr(g64, g64_exact))


def _grad_sizes():
    return {C64: GRAD_BOTH + (64,), C128: GRAD_BOTH + (40, "max")}


def _grad_n(n, cd):
    return _grad_max_n(cd) if n == "max" else n


def test_gradient_inputs_are_well_conditioned():
    """The eigenvector matrix (unit columns) of every gradient input keeps its lowest singular value above 1e-3: g_A = V^-H
    diag(g) V^H is then a well-posed solve, and what the test compares is the kernel's arithmetic, not an ill-conditioned basis"""
    for cd in (C64, C128):
        for n in _grad_sizes()[cd]:
            N = _grad_n(n, cd)
            for fam in GRAD_FAMILIES:
                V = torch.linalg.eig(_family(fam, N, cd))[1]
                V = V / torch.linalg.vector_norm(V, dim=-2, keepdim=True)
                assert torch.linalg.svdvals(V)[..., -1].min() > 1e-3, (fam, N, cd)
                c = _grad_case(fam, N)
                assert 0 < c["l2"] < 1e-3 and 0 < c["max"] < 1e-3, (fam, N, c["l2"], c["max"])


def _grad_params():
    return [pytest.param(n, cd, id=f"{n}-{_sfx(cd)}") for cd in (C64, C128) for n in _grad_sizes()[cd]]


@pytest.mark.gpu
@pytest.mark.parametrize("n,cd", _grad_params())
def test_gradients_against_float64_autograd(gpu, n, cd):
    """dL/dA through ops.eigvals (eigenvectors by back substitution, one LU solve per bin) against complex128 autograd through
    torch.linalg.eigvals on the CPU.  complex64: l2 and max-norm error at most 4 x those of the same autograd run in complex64
    on the CPU.  complex128: nothing wider exists to measure LAPACK's own error with, so the limit is the complex64 limit of the
    same family and size times 2^-29 (the ratio of the unit roundoffs).  N = 64 (complex64), 40 and the largest size the library
    accepts with eigenvectors (complex128: 57) are the three-matrix LDS layout above 64 KB."""
    from flamo_amd import ops
    N = _grad_n(n, cd)
    shrink = 1.0 if cd == C64 else 2.0 ** -29
    rep = _Report()
    for fam in GRAD_FAMILIES:
        c = _grad_case(fam, N)
        A = _family(fam, N, cd).to(gpu, cd).requires_grad_(True)
        (g,) = torch.autograd.grad(_loss(ops.eigvals(A)), [A])
        info = int(ops.eigvals_info().abs().max())
        name = f"eig_routes/{fam}_{N}_{_sfx(cd)}/g_A"
        rep.require(info == 0, f"{name}: eigvals_info() reports {info}")
        print(f"[grad] {name}: complex64 autograd on the CPU l2 {c['l2']:.3e} max {c['max']:.3e}; limits x {FACTOR * shrink:.3e}")
        rep.close(name, g.cpu().to(C128), c["ref"][cd], FACTOR * shrink * c["l2"], FACTOR * shrink * c["max"])
    rep.done()


@pytest.mark.gpu
def test_gradient_refused_one_above_the_largest_size(gpu):
    """complex128 that requires grad, one above the largest size whose three-matrix layout fits: the library's error, raised
    cleanly; the same input under no_grad (two matrices) succeeds, and so does N = 64"""
    from flamo_amd import ops
    N = _grad_max_n(C128) + 1
    A = _family("gauss", N, C128)
    Ad = A.to(gpu).requires_grad_(True)
    with pytest.raises(RuntimeError, match=rf"eig: N={N} does not fit in LDS at this precision"):
        ops.eigvals(Ad)
    torch.cuda.synchronize()
    rep = _Report()
    for n in (N, 64):
        lam, info = _kernel_spectrum(gpu, "gauss", n, C128)
        rep.spectrum(f"eig_routes/nograd_{n}_c128", "gauss", n, C128, lam, info)
    rep.done()
