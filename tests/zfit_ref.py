"""The Zernike wavefront fit from ray errors (metrics.zernike_moments / zernike_fit; tl_zfit_moments / tl_zfit_solve / tl_zfit_seed
of include/tl_trace.h) restated in float64 numpy from the definition, with the bounds the kernels are held to and a CPU emulation
of the kernels' summation order.  It shares no code with the package.

DEFINITION.  N = max_order, J = (N+1)(N+2)/2 - 1; Z_j, j = 2 .. J+1, the Noll-indexed Zernike polynomials, orthonormal over the
unit disc, p = rho cos(theta) along x, q = rho sin(theta) along y, even j the cosine terms.  A row is one (lens, field,
wavelength); a ray is live iff ok != 0.  Per row, over the live rays, a minimises
    sum (x - sum_j a_j dZ_j/dp)^2 + (y - sum_j a_j dZ_j/dq)^2,
here by numpy.linalg.lstsq on the 2n x J design matrix -- no normal equations.  G = A^T A, b = A^T (x; y), D = diag(G),
G^ = D^-1/2 G D^-1/2; the row is valid iff 2n >= J (so n >= 1), every D_jj > 0 and every pivot of the Cholesky factorisation of
G^ in natural order (the value whose root is the factor's diagonal) exceeds 2^-30; an invalid row has a = 0, q = 0.
q = sum (x^2 + y^2) - b . a.  The monomial sums: tri(a, b) = (a + b)(a + b + 1)/2 + b; M[tri(a,b)] = sum p^a q^b (a + b <= 2N - 2),
then sum x p^a q^b and sum y p^a q^b (a + b <= N - 1), then sum x^2, sum y^2; p^0 = 1, p^k = p^(k-1) p, a term (p^a q^b) then times x.

BOUNDS (U = 2^-53, derived, not measured).
  moments   |M_k - ref| <= (P + 8) U sum|term|, as tests/focus_ref.py derives it: both sides add the same fp64 terms (nothing is
            contracted, the order of a term's products is the definition's) in different orders.
  a         First-order perturbation of G^ a^ = b^ (a^ = D^1/2 a): |da^|_2 <= |G^^-1|_2 (|db^|_2 + |dG^|_F |a^|_2), with
            dG = |T|^T dG_m |T| entry by entry from the moment bounds through G_m[(a,b),(c,d)] = a c mu(a+c-2, b+d) + b d mu(a+c, b+d-2)
            and b_m = a xi(a-1, b) + b eta(a, b-1), plus what forming them costs: (2J + 8) U |T|^T |G_m| |T| for the two products
            of J terms, 4 J^2 U for the factorisation and the two triangular solves of a matrix with unit diagonal (|L||L^T| <= J),
            and 16 J U |G^^-1| |a^| for the reference's own lstsq.  Doubled, for the terms of second order.
            |da_j| <= D_jj^-1/2 |da^|_2 + 4 U |a_j|.
  q         the bounds of sum x^2 and sum y^2, |db| . |a| + |b| . |da|, and (J + 4) U (sum x^2 + sum y^2 + |b| . |a|).
  seeds     gx_i = 2 g_q x_i + sum_j bbar_j dZ_j/dp, bbar = G^-1 g_a - 2 g_q a.  s = G^-1 g_a is bounded as a is, with an exact
            right-hand side; |dbbar_j| <= |ds_j| + 2 |g_q| |da_j| + 4 U (|s_j| + |2 g_q a_j|).  The kernel evaluates the polynomial
            in MONOMIAL form by Horner, so the rounding term scales with the monomials' magnitudes:
            |dgx_i| <= 2^-24 |ref| + sum_j |dbbar_j| |dZ_j/dp| + 64 U (|2 g_q x_i| + sum_m (sum_j |T_mj| |bbar_j|) |d mono_m/dp|) + 2^-149
            (J <= 27 terms of the change of basis, <= 24 Horner steps, the seed's product and sum: below 64).
"""
import numpy as np

import rows_ref
from rows_ref import BLOCK, CHUNK, MAX_Y, TARGET_BLOCKS, VEC, plan        # noqa: F401 (the tests read them from here)

U = 2.0 ** -53
PIVOT_FLOOR = 2.0 ** -30


def sizes(order):
    return (order + 1) * (order + 2) // 2 - 1, 3 * order * order + 2


def tri(a, b):
    return (a + b) * (a + b + 1) // 2 + b


def monomials(top, lowest=0):
    """(a, b) with lowest <= a + b <= top, by degree, b ascending."""
    return [(d - b, b) for d in range(lowest, top + 1) for b in range(d + 1)]


def noll(j):
    """(n, m, sine) of Noll's index j >= 1."""
    n = 0
    while (n + 1) * (n + 2) // 2 < j:
        n += 1
    k = j - n * (n + 1) // 2
    m = 2 * (k // 2) if n % 2 == 0 else 2 * ((k - 1) // 2) + 1
    return n, m, m != 0 and j % 2 == 1


def zernike_polynomial(j, size):
    """c[a, b] (size x size): Z_j = sum c[a, b] p^a q^b, by polynomial multiplication: (p + i q)^m, times the radial polynomial in
    rho^2 = p^2 + q^2, times the norm."""
    from math import factorial
    n, m, sine = noll(j)
    mul_p = lambda c: np.pad(c, ((1, 0), (0, 0)))[:size]                          # noqa: E731
    mul_q = lambda c: np.pad(c, ((0, 0), (1, 0)))[:, :size]                       # noqa: E731
    re, im = np.zeros((size, size)), np.zeros((size, size))
    re[0, 0] = 1.0
    for _ in range(m):
        re, im = mul_p(re) - mul_q(im), mul_p(im) + mul_q(re)
    ang = im if sine else re
    out = np.zeros((size, size))
    for s in range((n - m) // 2 + 1):
        rc = (-1) ** s * factorial(n - s) / (factorial(s) * factorial((n + m) // 2 - s) * factorial((n - m) // 2 - s))
        term = ang
        for _ in range((n - m) // 2 - s):
            term = mul_p(mul_p(term)) + mul_q(mul_q(term))
        out += rc * term
    return out * np.sqrt(n + 1 if m == 0 else 2 * (n + 1))


def basis(order):
    """T [J, J]: Z_{j+2} = sum_m T[m, j] p^a_m q^b_m over monomials(order, 1) (the constant left out)."""
    J = sizes(order)[0]
    mono = monomials(order, 1)
    T = np.zeros((J, J))
    for j in range(2, J + 2):
        c = zernike_polynomial(j, order + 1)
        for i, (a, b) in enumerate(mono):
            T[i, j - 2] = c[a, b]
    return T


def powers(v, top):
    out = [np.ones_like(v)]
    for _ in range(top):
        out.append(out[-1] * v)
    return out


def clean(x, y, ok, px, py, dtype=np.float64):
    """The five arrays broadcast to [B,F,P,W], the dead rays at the origin of spot and pupil, and the live mask."""
    x, y, ok, px, py = np.broadcast_arrays(x, y, ok, px, py)
    live = ok != 0
    return tuple(np.where(live, a.astype(dtype), dtype(0)) for a in (x, y, px, py)) + (live,)


def ray_terms(x, y, ok, px, py, order, dtype=np.float64, wrong=None):
    """[B,F,P,W,K]: the K terms of every ray (zeros for a dead one), formed in `dtype` (float32: the wrong inner loop)."""
    x, y, p, q, live = clean(x, y, ok, px, py, dtype)
    if wrong == "swap_pq":
        p, q = q, p
    pp, qq = powers(p, 2 * order - 2), powers(q, 2 * order - 2)
    t = [live.astype(dtype) if (a, b) == (0, 0) else pp[a] * qq[b] for a, b in monomials(2 * order - 2)]
    t += [(pp[a] * qq[b]) * x for a, b in monomials(order - 1)] + [(pp[a] * qq[b]) * y for a, b in monomials(order - 1)]
    t += [x * x, y * y]
    t = np.stack(t, axis=-1).astype(np.float64)
    if wrong in ("drop", "twice"):
        first = np.flatnonzero(live.ravel())[live.sum() // 2]
        t.reshape(-1, t.shape[-1])[first] *= 0.0 if wrong == "drop" else 2.0
    return t


def moments(x, y, ok, px, py, order):
    """(M, T): M [B,F,W,K] and the sums of the terms' magnitudes."""
    t = ray_terms(x, y, ok, px, py, order)
    return t.sum(axis=2), np.abs(t).sum(axis=2)


def moment_bound(T, n_terms):
    return (n_terms + 8) * U * T


def gradients(p, q, order, T):
    """(dZ/dp, dZ/dq, dmono/dp, dmono/dq), each [..., J], at the points p, q."""
    pp, qq = powers(p, order), powers(q, order)
    mono = monomials(order, 1)
    zero = np.zeros_like(p)
    mp = np.stack([a * pp[a - 1] * qq[b] if a else zero for a, b in mono], axis=-1)
    mq = np.stack([b * pp[a] * qq[b - 1] if b else zero for a, b in mono], axis=-1)
    return mp @ T, mq @ T, mp, mq


def pivots(Gs):
    """The pivots of the Cholesky factorisation of Gs in natural order, as far as it runs (the first one <= 0 ends it)."""
    A = np.array(Gs, dtype=np.float64)
    J = len(A)
    out = []
    for k in range(J):
        d = A[k, k]
        out.append(d)
        if not d > 0:
            break
        A[k:, k] /= np.sqrt(d)
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
    return np.array(out)


def fit(x, y, ok, px, py, order, g_a=None, g_q=None):
    """dict of the reference and its bounds: M, T, M_bound [B,F,W,K]; n, valid, pivot (smallest), a, a_bound [.., J], q, q_bound;
    with seeds g_a [B,F,W,J], g_q [B,F,W] also gx, gy and their bounds [B,F,P,W]."""
    J, K = sizes(order)
    Tz = basis(order)
    aT = np.abs(Tz)
    mono = monomials(order, 1)
    x, y, p, q, live = clean(x, y, ok, px, py)
    B, F, P, W = x.shape
    M, T = moments(x, y, ok, px, py, order)
    Mb = moment_bound(T, P)
    nmu, nxi = order * (2 * order - 1), order * (order + 1) // 2
    out = dict(M=M, T=T, M_bound=Mb, n=M[..., 0], valid=np.zeros((B, F, W), bool), pivot=np.zeros((B, F, W)),
               a=np.zeros((B, F, W, J)), a_bound=np.zeros((B, F, W, J)), q=np.zeros((B, F, W)), q_bound=np.zeros((B, F, W)), P=P)
    seeded = g_a is not None
    if seeded:
        out.update({k: np.zeros((B, F, P, W)) for k in ("gx", "gy", "gx_bound", "gy_bound")})
    for r in np.ndindex(B, F, W):
        sel = (r[0], r[1], slice(None), r[2])
        lv = live[sel]
        n = int(lv.sum())
        if 2 * n < J:                                         # fewer equations than unknowns: G is singular
            continue
        xr, yr, pr, qr = x[sel][lv], y[sel][lv], p[sel][lv], q[sel][lv]
        Zp, Zq, mp, mq = gradients(pr, qr, order, Tz)
        A, rhs = np.concatenate([Zp, Zq]), np.concatenate([xr, yr])
        G, b = A.T @ A, A.T @ rhs
        D = np.diag(G)
        if not np.all(D > 0):
            continue
        isd = 1.0 / np.sqrt(D)
        Gs = G * isd[:, None] * isd[None, :]
        piv = pivots(Gs)
        out["pivot"][r] = piv.min()
        if len(piv) < J or not piv.min() > PIVOT_FLOOR:
            continue
        out["valid"][r] = True
        a = np.linalg.lstsq(A, rhs, rcond=None)[0]
        # the bound: moments -> G_m, b_m -> G, b -> the scaled system
        mu, e_mu = np.abs(M[r]), Mb[r]
        Gm, eGm = np.zeros((J, J)), np.zeros((J, J))
        bm, ebm = np.zeros(J), np.zeros(J)
        for i, (a1, b1) in enumerate(mono):
            for k, (c1, d1) in enumerate(mono):
                for w_, idx in ((a1 * c1, tri(a1 + c1 - 2, b1 + d1) if a1 * c1 else 0), (b1 * d1, tri(a1 + c1, b1 + d1 - 2) if b1 * d1 else 0)):
                    Gm[i, k] += w_ * mu[idx]
                    eGm[i, k] += w_ * e_mu[idx]
            for w_, idx in ((a1, nmu + tri(a1 - 1, b1) if a1 else 0), (b1, nmu + nxi + tri(a1, b1 - 1) if b1 else 0)):
                bm[i] += w_ * mu[idx]
                ebm[i] += w_ * e_mu[idx]
        eG = aT.T @ (eGm + 4 * U * Gm) @ aT + (2 * J + 8) * U * (aT.T @ Gm @ aT)
        eb = aT.T @ (ebm + 4 * U * bm) + (J + 8) * U * (aT.T @ bm)
        ninv = 1.0 / np.linalg.eigvalsh(Gs)[0]
        eGs = np.linalg.norm(eG * isd[:, None] * isd[None, :]) + 4 * J * J * U

        def solve_bound(sol, e_rhs):
            hat = sol / isd
            d_hat = 2 * ninv * (np.linalg.norm(e_rhs * isd) + (eGs + 16 * J * U) * np.linalg.norm(hat))
            return isd * d_hat + 4 * U * np.abs(sol)
        da = solve_bound(a, eb)
        out["a"][r], out["a_bound"][r] = a, da
        sxx = M[r][K - 2] + M[r][K - 1]
        out["q"][r] = sxx - b @ a
        out["q_bound"][r] = (Mb[r][K - 2] + Mb[r][K - 1] + eb @ np.abs(a) + np.abs(b) @ da
                             + (J + 4) * U * (sxx + np.abs(b) @ np.abs(a)))
        if seeded:
            ga, gq = g_a[r], g_q[r]
            s = np.linalg.solve(G, ga)
            ds = solve_bound(s, np.zeros(J))
            bbar = s - 2 * gq * a
            dbbar = ds + 2 * abs(gq) * da + 4 * U * (np.abs(s) + np.abs(2 * gq * a))
            spread = aT @ np.abs(bbar)                        # the monomial coefficients' magnitudes, uncancelled
            for key, Z, mo, v in (("gx", Zp, mp, xr), ("gy", Zq, mq, yr)):
                ref = 2 * gq * v + Z @ bbar
                bound = 2.0 ** -24 * np.abs(ref) + np.abs(Z) @ dbbar + 64 * U * (np.abs(2 * gq * v) + np.abs(mo) @ spread) + 2.0 ** -149
                full, fb = np.zeros(P), np.zeros(P)
                full[lv], fb[lv] = ref, bound
                out[key][sel], out[key + "_bound"][sel] = full, fb
    return out


def finish(a, q, n, valid, scale=1.0):
    """dict coeffs, rms, rms_focus, residual of the outputs' definitions."""
    c = np.asarray(scale, np.float64)[..., None] * a
    root = lambda v: np.sqrt(np.where(v > 0, v, 0.0))                             # noqa: E731
    return dict(coeffs=c, rms=root((c[..., 2:] ** 2).sum(-1)), rms_focus=root((c[..., 3:] ** 2).sum(-1)),
                residual=root(q / np.maximum(n, 1.0)))


# ---------------------------------------------------------------------------------------------------- the kernels, emulated
def workspace_bytes(F, P, W, order):
    return rows_ref.workspace_bytes(F, P, W, sizes(order)[1]) if order in (2, 3, 4, 5, 6) else 0


def emulate_moments(x, y, ok, px, py, order, aligned, dtype=np.float64, wrong=None):
    """M [B,F,W,K] in the kernels' order of summation: per lane in the order of its loop (four consecutive rays per step of 1024
    where aligned[row], else one per step of 256), the butterfly over the 64 lanes of a wave, the four waves in order, the
    row's partials in order.  dtype=float32 forms the per-ray terms in float32 (the sums stay float64)."""
    t = ray_terms(x, y, ok, px, py, order, dtype=dtype, wrong=wrong)
    B, F, P, W, K = t.shape
    t = np.ascontiguousarray(t.transpose(0, 1, 3, 2, 4)).reshape(B * F * W, P, K)
    out = rows_ref.emulate_sums(t, np.asarray(aligned))
    return out.reshape(B, F, W, K)
