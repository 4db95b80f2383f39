"""60-digit reference of the damped solve of one LM iteration, and the metric its result is held to. NOT a test file.

The system (csrc/teb_kernel.hpp, the `it == 0` branch and the trial loop; g2o's damped system over the non-fixed vertices):
  free variables  r in [3, 4 (n - 1)) in the order var(i, c) = 4 i + c: dt_0, the poses 1 .. n - 2, their dt
  lambda0 = fl(1e-5 max |H_rr|) over the free r; a rejected trial multiplies lambda by 2, 4, 8, .. (exact products), so the accepted
  trial k used lambda_k = lambda0 2^((k - 1) k / 2)
  A = H[free, free] + lambda_k I,  A dx = b[free]
Every vector here runs over the free variables only (entry j is variable 3 + j); H comes as its lower band (hp_linearize.band_of_dense:
column d of row a holds H[a, a - d]).

Arithmetic: the standard library's decimal at 60 digits. Decimal(float) is exact, and a banded LDL^T needs only + - x /. No mpmath: the
GPU test runs where it is absent. A band of 944 poses (3769 unknowns, half-width 10) costs ~ 2.5e5 multiplications to factor and
~ 8e4 per solve: 0.3 s and 0.1 s with the C implementation of decimal.

The metric.
  backward_error: omega_i = max(0, |r_i| - (|A| noise)_i) / ((|A| |step|)_i + |b_i|), r = A step - b in decimal, PER ROW: the unknowns
      mix metres, radians and seconds under weights from 1 to 1000, a norm over all rows would hide the light ones.
  forward_error:  max_i max(0, |step_i - dx_hp_i| - noise_i) / max_j |dx_hp_j|, over all variables and per kind (x / y, theta, dt).
  noise: the step is recovered from the states either side of the accepted trial. The trial adds its step once (x += dx, theta =
      normalize_theta(theta + dx), dt += dx), so after - before, evaluated exactly, is the solve's step up to the rounding of that one
      addition: at most ulp(after) / 2 per component.
"""
import math
from decimal import Decimal, localcontext

import numpy as np

from hp_linearize import BAND

DIGITS = 60
EPS = float(np.finfo(np.float64).eps)
KINDS = ("xy", "theta", "dt")


def kind_of(r):
    """variable kind of the canonical index r = 4 i + c"""
    return ("xy", "xy", "theta", "dt")[r & 3]


def lambda_of(Hband, n, k):
    """lambda of the accepted trial k >= 1, exactly as the kernel has it (an fp64 product, then exact powers of two)"""
    assert k >= 1
    lo, hi = 3, 4 * (n - 1)
    lam0 = 1e-5 * float(np.abs(np.asarray(Hband)[lo:hi, 0]).max())
    lam = lam0 * float(2 ** ((k - 1) * k // 2))
    assert math.isfinite(lam)
    return lam


class System:
    """A = H[free, free] + lambda I as a decimal lower band, b[free], and the banded LDL^T of A (factored on first use)"""

    def __init__(self, Hband, b, n, lam, full=False, drop=None):
        """full: the system over ALL 4 n - 1 variables (fixed ones included) - only for the mutation checks; drop = (a, c): the entry
        A[a, c] (free-variable indices, a > c) is zeroed - likewise"""
        lo, hi = (0, 4 * n - 1) if full else (3, 4 * (n - 1))
        self.n, self.lo, self.N = n, lo, hi - lo
        Hband = np.asarray(Hband, dtype=np.float64)
        with localcontext() as c:
            c.prec = DIGITS
            lamd = Decimal(float(lam))
            self.A = []
            for j in range(self.N):
                row = [Decimal(float(Hband[lo + j, d])) for d in range(min(j, BAND) + 1)]
                row[0] += lamd
                self.A.append(row)
            if drop is not None:
                a, cc = drop
                assert 0 < a - cc <= BAND
                self.A[a][a - cc] = Decimal(0)
            self.b = [Decimal(float(v)) for v in np.asarray(b, dtype=np.float64)[lo:hi]]
        self._L = None

    def factor(self):
        if self._L is not None:
            return
        N, A = self.N, self.A
        with localcontext() as c:
            c.prec = DIGITS
            L = [[Decimal(1)] for _ in range(N)]   # L[i][d] = L[i, i - d]
            D = [Decimal(0)] * N
            for i in range(N):
                w = min(i, BAND)
                Li = [Decimal(0)] * (w + 1)
                Li[0] = Decimal(1)
                # entries of row i left to right: L[i, j], j = i - w .. i - 1, then the pivot
                for d in range(w, 0, -1):
                    j = i - d
                    s = A[i][d]
                    Lj = L[j]
                    for k in range(max(i - w, j - min(j, BAND)), j):
                        s -= Li[i - k] * Lj[j - k] * D[k]
                    Li[d] = s / D[j]
                s = A[i][0]
                for d in range(1, w + 1):
                    s -= Li[d] * Li[d] * D[i - d]
                if not s > 0:
                    raise ArithmeticError("pivot %d of the damped system is not positive: %s" % (i, s))
                D[i] = s
                L[i] = Li
            self._L, self._D = L, D

    def solve(self, rhs=None):
        self.factor()
        N, L, D = self.N, self._L, self._D
        with localcontext() as c:
            c.prec = DIGITS
            x = list(self.b if rhs is None else rhs)
            for i in range(N):
                Li, s = L[i], x[i]
                for d in range(1, len(Li)):
                    s -= Li[d] * x[i - d]
                x[i] = s
            for i in range(N):
                x[i] = x[i] / D[i]
            for i in range(N - 1, -1, -1):
                Li, xi = L[i], x[i]
                for d in range(1, len(Li)):
                    x[i - d] -= Li[d] * xi
            return x

    def matvec(self, v, absolute=False):
        """A v (or |A| v) in decimal"""
        N, A = self.N, self.A
        with localcontext() as c:
            c.prec = DIGITS
            out = [Decimal(0)] * N
            for i in range(N):
                Ai = A[i]
                for d in range(len(Ai)):
                    a = abs(Ai[d]) if absolute else Ai[d]
                    out[i] += a * v[i - d]
                    if d:
                        out[i - d] += a * v[i]
            return out

    def norm_inf(self):
        return max(self.matvec([Decimal(1)] * self.N, absolute=True))

    def inverse_norm_estimate(self, sweeps=5):
        """Hager's estimate of ||A^-1||_1 = ||A^-1||_inf (A is symmetric) from the 60-digit factorisation: a lower bound that is exact
        or within a small factor in practice - a bound FLOOR x kappa built on it errs on the strict side"""
        N = self.N
        with localcontext() as c:
            c.prec = DIGITS
            x = [Decimal(1) / N] * N
            est = Decimal(0)
            for _ in range(sweeps):
                y = self.solve(x)
                e = sum(abs(v) for v in y)
                if e <= est:
                    break
                est = e
                z = self.solve([Decimal(1) if v >= 0 else Decimal(-1) for v in y])
                j = max(range(N), key=lambda q: abs(z[q]))
                if abs(z[j]) <= sum(a * b for a, b in zip(z, x)):
                    break
                x = [Decimal(0)] * N
                x[j] = Decimal(1)
            # Higham's alternating vector guards against the estimator's known blind spots
            alt = [Decimal((-1) ** q) * (1 + Decimal(q) / max(N - 1, 1)) for q in range(N)]
            e2 = 2 * sum(abs(v) for v in self.solve(alt)) / (3 * N)
            return max(est, e2)

    def kappa(self):
        return float(self.norm_inf() * self.inverse_norm_estimate())

    def dense(self):
        """A as an fp64 matrix (every entry is H's own fp64 value; the diagonal fl(H_rr + lambda)) and b: what an fp64 solver is given"""
        N = self.N
        M = np.zeros((N, N))
        for i in range(N):
            for d in range(len(self.A[i])):
                M[i, i - d] = M[i - d, i] = float(self.A[i][d])
        return M, np.array([float(v) for v in self.b])


def reference_step(Hband, b, n, k, system=False):
    """(lambda_k, dx_hp): the accepted trial's lambda and the 60-digit solution of the damped system over the free variables;
    system=True also returns the factored System (condition estimate, fp64 twin, residuals)"""
    lam = lambda_of(Hband, n, k)
    S = System(Hband, b, n, lam)
    dx = S.solve()
    return (lam, dx, S) if system else (lam, dx)


def _dec(v):
    return [x if isinstance(x, Decimal) else Decimal(float(x)) for x in v]


def backward_error(Hband, b, n, lambda_k, step, noise, S=None):
    """omega per free row (fp64 array). A row with (|A| |step|)_i + |b_i| = 0 must have r_i = 0 exactly and gives 0."""
    S = S or System(Hband, b, n, lambda_k)
    step, noise = _dec(step), _dec(noise)
    with localcontext() as c:
        c.prec = DIGITS
        Ax = S.matvec(step)
        An = S.matvec(noise, absolute=True)
        Aa = S.matvec([abs(v) for v in step], absolute=True)
        out = np.zeros(S.N)
        for i in range(S.N):
            r = abs(Ax[i] - S.b[i])
            num = max(Decimal(0), r - An[i])
            den = Aa[i] + abs(S.b[i])
            if den == 0:
                assert num == 0, ("row with no scale carries a residual", i)
                continue
            out[i] = float(num / den)
        return out


def noise_share(Hband, b, n, lambda_k, step, noise, S=None):
    """max_i (|A| noise)_i / ((|A| |step|)_i + |b_i|): how much of the metric's scale the rounding of the state update may take"""
    S = S or System(Hband, b, n, lambda_k)
    step, noise = _dec(step), _dec(noise)
    with localcontext() as c:
        c.prec = DIGITS
        An = S.matvec(noise, absolute=True)
        Aa = S.matvec([abs(v) for v in step], absolute=True)
        worst = 0.0
        for i in range(S.N):
            den = Aa[i] + abs(S.b[i])
            if den == 0:
                continue
            worst = max(worst, float(An[i] / den))
        return worst


def forward_error(step, dx_hp, noise, n=None):
    """(overall, {kind: value}): max_i max(0, |step_i - dx_hp_i| - noise_i) / max_j |dx_hp_j|; per kind both maxima run over the
    variables of that kind. n is needed for the per-kind split only."""
    step, dx_hp, noise = _dec(step), _dec(dx_hp), _dec(noise)
    with localcontext() as c:
        c.prec = DIGITS
        err = [max(Decimal(0), abs(s - x) - e) for s, x, e in zip(step, dx_hp, noise)]
        scale = max(abs(x) for x in dx_hp)
        overall = float(max(err) / scale) if scale != 0 else (0.0 if max(err) == 0 else math.inf)
        per = {}
        if n is not None:
            assert len(step) == 4 * n - 7
            for kd in KINDS:
                idx = [j for j in range(len(step)) if kind_of(3 + j) == kd]
                sc = max(abs(dx_hp[j]) for j in idx)
                e = max(err[j] for j in idx)
                per[kd] = float(e / sc) if sc != 0 else (0.0 if e == 0 else math.inf)
        return overall, per


def recovered_step(before, after, n):
    """(step, noise) over the free variables, exactly: step = after - before in decimal, noise = ulp(after) / 2.
    before / after: (x, y, theta, dt) of the band either side of the one LM iteration. Raises if a fixed variable moved (start and goal
    pose are fixed vertices) or if a heading wrapped (then after - before is not the step)."""
    bx, by, bt, bd = (np.asarray(a, dtype=np.float64) for a in before)
    ax, ay, at, ad = (np.asarray(a, dtype=np.float64) for a in after)
    assert len(bx) == len(ax) == n and len(bd) >= n - 1 and len(ad) >= n - 1
    for i in (0, n - 1):
        for u, v, what in ((bx, ax, "x"), (by, ay, "y"), (bt, at, "theta")):
            if u[i] != v[i]:
                raise ValueError("fixed variable %s of pose %d moved: %r -> %r" % (what, i, u[i], v[i]))
    step, noise = [], []
    with localcontext() as c:
        c.prec = DIGITS

        def put(u, v):
            step.append(Decimal(float(v)) - Decimal(float(u)))
            noise.append(Decimal(math.ulp(float(v))) / 2)

        for i in range(n - 1):
            if i >= 1:
                if not (abs(at[i]) < math.pi and abs(at[i] - bt[i]) < math.pi):
                    raise ValueError("heading of pose %d wrapped: %r -> %r" % (i, bt[i], at[i]))
                put(bx[i], ax[i]); put(by[i], ay[i]); put(bt[i], at[i])
            put(bd[i], ad[i])
    assert len(step) == 4 * n - 7
    return step, noise


def fp64_twin(S):
    """what numpy.linalg.solve (LAPACK, fp64) gives on the same A and b: the yardstick of the bounds"""
    M, bv = S.dense()
    return np.linalg.solve(M, bv)


FLOOR = 256 * EPS


def bounds(Hband, b, n, lambda_k, dx_hp, S):
    """(bound_omega, bound_fwd, omega_cpu, fwd_cpu, kappa): max(FLOOR, 16 omega_cpu) and max(FLOOR kappa, 16 fwd_cpu), measured on the
    fp64 LAPACK solve of the same system under the same metric (its solution never went through a state update: its noise is 0)"""
    x = fp64_twin(S)
    zero = [Decimal(0)] * S.N
    omega_cpu = float(backward_error(Hband, b, n, lambda_k, x, zero, S).max())
    fwd_cpu = forward_error(x, dx_hp, zero)[0]
    kappa = S.kappa()
    return max(FLOOR, 16 * omega_cpu), max(FLOOR * kappa, 16 * fwd_cpu), omega_cpu, fwd_cpu, kappa


def check(Hband, b, n, k, before, after):
    """The whole check of one LM step, shared by the CPU test (oracle as the device) and the GPU test. Returns a dict of figures; the
    caller asserts omega <= bound_omega and fwd <= bound_fwd."""
    lam, dx_hp, S = reference_step(Hband, b, n, k, system=True)
    step, noise = recovered_step(before, after, n)
    om = backward_error(Hband, b, n, lam, step, noise, S)
    fwd, per = forward_error(step, dx_hp, noise, n)
    bo, bf, ocpu, fcpu, kappa = bounds(Hband, b, n, lam, dx_hp, S)
    worst = int(om.argmax())
    return dict(lam=lam, k=k, omega=float(om.max()), omega_row=3 + worst, omega_rows=om, fwd=fwd, fwd_kind=per, bound_omega=bo,
                bound_fwd=bf, omega_cpu=ocpu, fwd_cpu=fcpu, kappa=kappa, noise_share=noise_share(Hband, b, n, lam, step, noise, S),
                step=step, noise=noise, dx_hp=dx_hp, system=S)


def report(name, F):
    return ("%s: k %d lambda %.3e kappa %.2e | omega %.2f eps at row %d (bound %.0f, LAPACK %.2f) | forward %.3g eps "
            "(bound %.3g, LAPACK %.3g; x/y %.3g theta %.3g dt %.3g) | noise share %.2f eps" % (
                name, F["k"], F["lam"], F["kappa"], F["omega"] / EPS, F["omega_row"], F["bound_omega"] / EPS, F["omega_cpu"] / EPS,
                F["fwd"] / EPS, F["bound_fwd"] / EPS, F["fwd_cpu"] / EPS, F["fwd_kind"]["xy"] / EPS, F["fwd_kind"]["theta"] / EPS,
                F["fwd_kind"]["dt"] / EPS, F["noise_share"] / EPS))
