"""
References of tl_pupil_position (the paraxial entrance-pupil position z = B / A of the rows in front of the stop, and its
gradient), for tests/test_gpu_pupil_matrix.py and tests/test_aim_cases_cpu.py.  c, t [B,K], n [B,K+1] (n[:,0] the index in
front of row 0), plain numpy.

  tree32      strict mode.  The pairwise fp32 product tree of paraxial.reduce_abcd over interface_propagation_abcd, every
              product and sum rounded on its own (numpy float32 scalars-as-arrays never fuse), an odd count carrying its last
              matrix up a level: the torch CPU fp32 chain bit for bit (test_aim_cases_cpu.py), for every K.
  fast64      fast mode: the ordered float64 product M_{K-1} ... M_0 and b / a.
  grads64     float64 gradients of sum(g_z z) to c, t and n[0..K] by torch autograd on the float64 chain.
  kernel_order  pupil_position_kernel (csrc/tl_api.hip) in float64 with a first-order bound of the rounding error of every
              result, element by element -- the allowance of the tests.

THE ALLOWANCE.  The kernel carries the product of the row matrices up (R_k = M_{k-1} ... M_0) and the adjoint down
(G_k = L_k^T G, L_k = M_{K-1} ... M_{k+1}).  One step of either recurrence is, per entry, at most ROW = 7 roundings: r (1),
r - 1 (2), P = c (r - 1) (3), P t (4), 1 + P t (5), the product with the carried entry (6), the sum (7) -- on the seeded
fronts |r - 1| >= |r| / 3 or r = 1 exactly, so the subtraction costs no more than that.  What row m injects is therefore at
most 7 * 2^-53 |M_m| |before m|, and it reaches the end of the chain through the signed product of the rows after it:

    E(product) = 7 * 2^-53 * sum_m |rows after m| |M_m| |rows before m|        (entry by entry, |.| of 2 x 2 matrices)

-- the sum of the absolute terms of the chain; it grows with K like the chain itself, not like a product of absolute
matrices.  From a, b, R_k and L_k with these bounds each result is a handful of operations (z = b / a; G = (-g_z b / a^2,
g_z / a); dM_k = G_k R_k^T; dP, dt, dr; g_c, g_t, g_n), and Err arithmetic carries the bound through them: each operation adds
2^-53 |result|, a product |x| e_y + |y| e_x, a quotient e_x / |y| + |x| e_y / y^2.  An element of g_n is 13 such operations
past dM_k, one of g_c 6, z one.  The tests allow TWICE the bound: the float64 value it is compared with (another order,
autograd) went through as many roundings.

    |z_fast - z64| <= 2^-24 |z64| + 2 e(z)
    |g - g64|      <= 2^-24 |g64| + 2 e(g)                   for every element of g_c, g_t, g_n[0..K]
"""
import numpy as np
import torch

U64 = 2.0 ** -53
U32 = 2.0 ** -24


def tree32(c, t, n):
    """Strict mode's z [B] float32: pupil_position_fp32_tree / reduce_abcd in numpy float32."""
    c, t, n = (np.asarray(v, dtype=np.float32) for v in (c, t, n))
    K = c.shape[1]
    one = np.float32(1.0)
    r = n[:, :-1] / n[:, 1:]
    P = c * (r - one)
    M = [[one + P[:, k] * t[:, k], r[:, k] * t[:, k], P[:, k], r[:, k]] for k in range(K)]
    while len(M) > 1:
        cnt = len(M)
        even = cnt - (cnt & 1)
        nxt = []
        for i in range(0, even, 2):                  # out = M[i+1] @ M[i]
            a0, a1, a2, a3 = M[i + 1]
            b0, b1, b2, b3 = M[i]
            nxt.append([a0 * b0 + a1 * b2, a0 * b1 + a1 * b3, a2 * b0 + a3 * b2, a2 * b1 + a3 * b3])
        if cnt & 1:
            nxt.append(M[cnt - 1])
        M = nxt
    z = M[0][1] / M[0][0]
    assert z.dtype == np.float32
    return z


def fast64(c, t, n):
    """Fast mode's z before its rounding: the ordered float64 product, b / a, [B]."""
    c, t, n = (np.asarray(v, dtype=np.float64) for v in (c, t, n))
    B, K = c.shape
    a, b, cc, d = np.ones(B), np.zeros(B), np.zeros(B), np.ones(B)
    for k in range(K):
        r = n[:, k] / n[:, k + 1]
        P = c[:, k] * (r - 1.0)
        m00, m01, m10, m11 = 1.0 + P * t[:, k], r * t[:, k], P, r
        a, b, cc, d = m00 * a + m01 * cc, m00 * b + m01 * d, m10 * a + m11 * cc, m10 * b + m11 * d
    return b / a


def grads64(c, t, n, g_z):
    """(z, g_c, g_t, g_n) in float64 by autograd on the ordered float64 chain, for the cotangent g_z [B]."""
    c, t, n = (torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for v in (c, t, n))
    B, K = c.shape
    one, zero = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    a, b, cc, d = one, zero, zero, one
    for k in range(K):
        r = n[:, k] / n[:, k + 1]
        P = c[:, k] * (r - 1.0)
        m00, m01, m10, m11 = 1.0 + P * t[:, k], r * t[:, k], P, r
        a, b, cc, d = m00 * a + m01 * cc, m00 * b + m01 * d, m10 * a + m11 * cc, m10 * b + m11 * d
    z = b / a
    (z * torch.tensor(np.asarray(g_z, dtype=np.float64))).sum().backward()
    return z.detach().numpy(), c.grad.numpy(), t.grad.numpy(), n.grad.numpy()


class Err:
    """A float64 value [B] with a first-order bound `e` of its rounding error (running error analysis): every operation
    adds 2^-53 |result| to what its operands bring, x y brings |x| e_y + |y| e_x, x / y brings e_x / |y| + |x| e_y / y^2."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else e

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.of(o)
        v = self.v + o.v
        return Err(v, self.e + o.e + U64 * np.abs(v))

    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o)
        v = self.v - o.v
        return Err(v, self.e + o.e + U64 * np.abs(v))

    def __rsub__(self, o):
        return Err.of(o) - self

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        o = Err.of(o)
        v = self.v * o.v
        return Err(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U64 * np.abs(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        v = self.v / o.v
        return Err(v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v) + U64 * np.abs(v))


ROW = 7          # roundings on one entry of a step of the recurrence: r, r - 1, c (r - 1), P t, 1 + P t, the product, the sum


def _rows(c, t, n):
    """The row matrices M_k [B,2,2] float64, as a list."""
    r = n[:, :-1] / n[:, 1:]
    P = c * (r - 1.0)
    return [np.stack((np.stack((1.0 + P[:, k] * t[:, k], r[:, k] * t[:, k]), -1), np.stack((P[:, k], r[:, k]), -1)), -2)
            for k in range(c.shape[1])]


def chain_bounds(c, t, n):
    """The partial products the kernel carries and the bound of their rounding error, element by element:
    R[k] = M_{k-1} ... M_0 (k = 0..K; R[K] is the whole product) and L[k] = M_{K-1} ... M_{k+1}, each [B,2,2], with
    E = ROW 2^-53 sum_m |after m| |M_m| |before m| over the rows m of the product: the error a row's step injects is at
    most ROW roundings of |M_m| |before m|, and it reaches the end through the SIGNED product of the rows after it."""
    c, t, n = (np.asarray(v, dtype=np.float64) for v in (c, t, n))
    B, K = c.shape
    M = _rows(c, t, n)
    eye = np.broadcast_to(np.eye(2), (B, 2, 2))
    S = {}                                            # S[i, j] = M_j ... M_i (identity for j < i)
    for i in range(K + 1):
        S[i, i - 1] = eye
        for j in range(i, K):
            S[i, j] = M[j] @ S[i, j - 1]
    A = np.abs
    R = [S[0, k - 1] for k in range(K + 1)]
    L = [S[k + 1, K - 1] for k in range(K)]
    zero = np.zeros((B, 2, 2))
    E_R = [ROW * U64 * sum((A(S[m + 1, k - 1]) @ A(M[m]) @ A(S[0, m - 1]) for m in range(k)), zero) for k in range(K + 1)]
    E_L = [ROW * U64 * sum((A(S[m + 1, K - 1]) @ A(M[m]) @ A(S[k + 1, m - 1]) for m in range(k + 1, K)), zero)
           for k in range(K)]
    return R, E_R, L, E_L


def kernel_order(c, t, n, g_z):
    """pupil_position_kernel's float64 results with a bound of their rounding error: (z, g_c [K], g_t [K], g_n [K+1]) as
    Err numbers (lists over rows of Err [B]).  The forward recurrence and G_k = L_k^T G come from chain_bounds (values in
    the kernel's order, errors through the signed partial products); everything the kernel does per row on top of them is
    redone here operation for operation on Err numbers."""
    c, t, n = (np.asarray(v, dtype=np.float64) for v in (c, t, n))
    B, K = c.shape
    R, E_R, L, E_L = chain_bounds(c, t, n)
    a, b = Err(R[K][:, 0, 0], E_R[K][:, 0, 0]), Err(R[K][:, 0, 1], E_R[K][:, 0, 1])
    z = b / a
    gz = Err(np.asarray(g_z, dtype=np.float64))
    G0 = (-gz * b / (a * a), gz / a)                  # the first row of G; its second row is zero
    g_c, g_t, g_n = [None] * K, [None] * K, [None] * (K + 1)
    carry = Err(np.zeros(B))
    for k in range(K - 1, -1, -1):
        nk, nk1 = Err(n[:, k]), Err(n[:, k + 1])
        r, ck, tk = nk / nk1, Err(c[:, k]), Err(t[:, k])
        P = ck * (r - 1.0)
        Lk = [[Err(L[k][:, i, j], E_L[k][:, i, j]) for j in range(2)] for i in range(2)]
        Rk = [[Err(R[k][:, i, j], E_R[k][:, i, j]) for j in range(2)] for i in range(2)]
        # G_k = L_k^T G: G_k[i][j] = L_k[0][i] G0[j]
        G00, G01, G10, G11 = Lk[0][0] * G0[0], Lk[0][0] * G0[1], Lk[0][1] * G0[0], Lk[0][1] * G0[1]
        d00, d01 = G00 * Rk[0][0] + G01 * Rk[0][1], G00 * Rk[1][0] + G01 * Rk[1][1]
        d10, d11 = G10 * Rk[0][0] + G11 * Rk[0][1], G10 * Rk[1][0] + G11 * Rk[1][1]
        dP = d00 * tk + d10
        dt = d00 * P + d01 * r
        dr = d01 * tk + d11 + dP * ck
        g_c[k] = dP * (r - 1.0)
        g_t[k] = dt
        g_n[k + 1] = carry - dr * nk / (nk1 * nk1)
        carry = dr / nk1
    g_n[0] = carry
    return z, g_c, g_t, g_n


def stacked(errs):
    """A list over rows of Err [B] -> (values [B,rows], error bounds [B,rows])."""
    return np.stack([q.v for q in errs], axis=1), np.stack([q.e for q in errs], axis=1)


def seeded_front(K, B, seed, padded=False):
    """A seeded batch of fronts, fp32 values: weak random curvatures, gaps 0.5 .. 3.5, glass (1.45 .. 1.9) and air in turn.
    padded (K >= 2): lens b keeps its first 2 (1 + (7 b + 3) % (K // 2)) rows -- an even count, so its stop sits in air -- and
    the rows behind are identity (c = 0, t = 0, n = 1)."""
    rng = np.random.default_rng(seed)
    c = ((rng.random((B, K)) - 0.5) * 0.05).astype(np.float32)
    t = (rng.random((B, K)) * 3 + 0.5).astype(np.float32)
    glass = (1.45 + 0.45 * rng.random((B, K))).astype(np.float32)
    n = np.ones((B, K + 1), dtype=np.float32)
    n[:, 1:] = np.where(np.arange(K)[None, :] % 2 == 0, glass, np.float32(1.0))
    if padded and K >= 2:
        keep = 2 * (1 + (7 * np.arange(B) + 3) % (K // 2))
        behind = np.arange(K)[None, :] >= keep[:, None]
        c[behind], t[behind] = 0.0, 0.0
        n[:, 1:][behind] = 1.0
    return c, t, n
