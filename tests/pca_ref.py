"""Independent restatement of the per-recording PCA of the dense PLDA scores with the number format
as a parameter (numpy.float64 or numpy.longdouble), its own cyclic Jacobi eigensolver, Cholesky factorisation and Gauss-Jordan
inverse (numpy.linalg has no longdouble), the seeded generator of the test cases, and the tolerance rule: a quantity of one recording
is held to M * e64 + floor, e64 the largest difference between the float64 and the longdouble run of this restatement on the same
input, floor 16 ulp (2^-52) of the quantity's largest magnitude."""
import numpy as np

LD = np.longdouble
M = 32                      # the next power of two at least 4 times the largest ratio measured (6.66)
ULP = 2.0 ** -52
# (n, L, K): rows, dimensions, planted speakers
CASES = [(2, 4, 1), (3, 5, 2), (17, 16, 3), (33, 17, 3), (65, 40, 4), (130, 128, 4), (257, 150, 4)]
ENERGIES = [0.1, 0.5, 0.9]


# ---- linear algebra in any format --------------------------------------------------------------------------------------------------
def jacobi(A, dtype, max_sweeps=60):
    """cyclic Jacobi on the symmetric A, the pairs of one round-robin round rotated together -> (w descending, V with columns the
    eigenvectors, sweeps)"""
    A = np.array(A, dtype=dtype)
    m = A.shape[0]
    if m == 1:
        return A[0].copy(), np.ones((1, 1), dtype=dtype), 0
    pad = m & 1
    if pad:
        A = np.pad(A, ((0, 1), (0, 1)))
    me = m + pad
    V = np.eye(me, dtype=dtype)
    eps = np.finfo(dtype).eps
    ring = np.arange(me - 1)
    one = dtype(1)
    for sweep in range(max_sweeps):
        off = A - np.diag(np.diag(A))
        if not np.abs(off).max() > eps * dtype(1e-3) * np.abs(np.diag(A)).max():
            break
        for r in range(me - 1):
            rot = np.roll(ring, -r)
            a = np.concatenate([[me - 1], rot[1:me // 2]])
            b = np.concatenate([[rot[0]], rot[:me // 2 - 1:-1]])
            p, q = np.minimum(a, b), np.maximum(a, b)
            apq = A[p, q]
            live = apq != 0
            safe = np.where(live, apq, one)
            theta = (A[q, q] - A[p, p]) / (2 * safe)
            t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
            t = np.where(live, t, 0 * one)
            c = one / np.sqrt(t * t + one)
            s = t * c
            Ap, Aq = A[p, :].copy(), A[q, :].copy()
            A[p, :] = c[:, None] * Ap - s[:, None] * Aq
            A[q, :] = s[:, None] * Ap + c[:, None] * Aq
            Ap, Aq = A[:, p].copy(), A[:, q].copy()
            A[:, p] = c[None, :] * Ap - s[None, :] * Aq
            A[:, q] = s[None, :] * Ap + c[None, :] * Aq
            A[p, q] = 0
            A[q, p] = 0
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p] = c[None, :] * Vp - s[None, :] * Vq
            V[:, q] = s[None, :] * Vp + c[None, :] * Vq
    w = np.diag(A)[:m].copy()
    order = np.argsort(-w, kind="stable")
    return w[order], V[:m, :m][:, order], sweep


def cholesky(A, dtype):
    """lower G with G G^T = A, or None when a pivot is not positive"""
    A = np.array(A, dtype=dtype)
    m = A.shape[0]
    G = np.zeros((m, m), dtype=dtype)
    for j in range(m):
        v = A[j:, j] - G[j:, :j] @ G[j, :j]
        if not v[0] > 0:
            return None
        G[j:, j] = v / np.sqrt(v[0])
    return G


def inverse(A, dtype):
    """Gauss-Jordan with row pivoting"""
    A = np.array(A, dtype=dtype)
    m = A.shape[0]
    X = np.eye(m, dtype=dtype)
    for j in range(m):
        k = j + int(np.argmax(np.abs(A[j:, j])))
        if k != j:
            A[[j, k]] = A[[k, j]]
            X[[j, k]] = X[[k, j]]
        piv = A[j, j]
        A[j] = A[j] / piv
        X[j] = X[j] / piv
        f = A[:, j].copy()
        f[j] = 0
        A -= f[:, None] * A[j][None, :]
        X -= f[:, None] * X[j][None, :]
    return X


def dense_terms(psi):
    g = psi / (2 * psi + 1)
    k = psi * psi / ((psi + 1) * (2 * psi + 1))
    K = (np.log(psi + 1) - np.log(1 + psi / (psi + 1))).sum() / 2
    return g, k, K


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def dim_rule(s, n, E):
    """the retained dimension, stated directly: None = the recording skips the PCA"""
    L = len(s)
    tot = s[0] * 0
    for v in s:
        tot = tot + v
    if n == 1 or not tot > 0:
        return None
    cum = s[0] * 0
    for k in range(1, L + 1):
        cum = cum + s[k - 1]
        if cum / tot > E:
            return min(k + 1, L, n - 1)
    raise AssertionError("cum_L == tot")


_EIG = {}


def cov_eig(z, dtype):
    """steps 1 and 2, shared by every E: (s floored at 0 and descending, P with columns the eigenvectors)"""
    key = (z.shape, z.tobytes(), np.dtype(dtype).name)
    if key not in _EIG:
        x = z.astype(dtype)
        n = x.shape[0]
        mu = x.sum(axis=0) / n
        C = (x.T @ x) / n - np.outer(mu, mu)
        C = (C + C.T) / 2
        if dtype is LD and C.shape[0] >= 64:
            # the longdouble iteration started from the float64 basis of numpy.linalg.eigh: the rotations that are left are small,
            # and the result is the longdouble Jacobi's own (a third of the sweeps at these orders)
            V0 = np.linalg.eigh(C.astype(np.float64))[1].astype(LD)
            V0 = V0 @ (3 * np.eye(len(V0), dtype=LD) - V0.T @ V0) / 2       # one Newton-Schulz step: orthonormal to 2^-100
            A0 = V0.T @ C @ V0
            s, P, _ = jacobi((A0 + A0.T) / 2, dtype)
            P = V0 @ P
        else:
            s, P, _ = jacobi(C, dtype)
        _EIG[key] = (np.maximum(s, 0), P)
    return _EIG[key]


def project_model(P_r, model, dtype):
    """steps 4 and 5 for the rows P_r [dim][L] -> (psi_r [dim], A_r [dim][L], W, B), or None for a non-positive pivot"""
    m, T, psi = (np.asarray(v).astype(dtype) for v in model)
    Ti = inverse(T, dtype)
    W, B = Ti @ Ti.T, (Ti * psi[None, :]) @ Ti.T
    Wr, Br = P_r @ W @ P_r.T, P_r @ B @ P_r.T
    G = cholesky((Wr + Wr.T) / 2, dtype)
    if G is None:
        return None
    T1 = inverse(G, dtype)
    Mr = T1 @ Br @ T1.T
    p, U, _ = jacobi((Mr + Mr.T) / 2, dtype)
    return np.maximum(p, 0), U.T @ T1 @ P_r, W, B


def rows_and_scores(z, A, b, psi_r, dim, dtype, normalize_length=True, simple=False):
    """steps 6 and 7 -> (u [n][dim], S [n][n]) in dtype"""
    u = z.astype(dtype) @ A.T + b
    if normalize_length:
        wgt = np.ones(dim, dtype=dtype) if simple else 1 / (psi_r + 1)
        ss = (u * u * wgt[None, :]).sum(axis=1)
        u = u * np.where(ss > 0, np.sqrt(dim / np.where(ss > 0, ss, 1)), 1)[:, None]
    g, k, K = dense_terms(psi_r)
    q = -(k[None, :] * u * u).sum(axis=1) / 2
    return u, (u * g[None, :]) @ u.T + q[:, None] + q[None, :] + K


def pca_ref(z, model, E, dtype, normalize_length=True, simple=False):
    """steps 1-7 for the float32 rows z [n][L] of one recording and the smoothed model (m, T, psi) -> dict(dim, skip, s, psi_r, A, b,
    u, S, P) in dtype; A, b, psi_r and u have dim rows / entries (no padding)"""
    n, L = z.shape
    m, T, psi = (np.asarray(v).astype(dtype) for v in model)
    s, P = cov_eig(z, dtype)
    dim = dim_rule(s, n, E)
    if dim is None:
        A, psi_r, dim, skip = T, psi, L, True
    else:
        psi_r, A, _, _ = project_model(P[:, :dim].T, model, dtype)
        skip = False
    b = -(A @ m)
    u, S = rows_and_scores(z, A, b, psi_r, dim, dtype, normalize_length, simple)
    return {"dim": dim, "skip": skip, "s": s, "psi_r": psi_r, "A": A, "b": b, "u": u, "S": S, "P": P}


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def planted(n, L, K, seed=0):
    """-> (z [n][L] float32, labels [n], model (m, T, psi) float64): rows = speaker + noise, both scaled per dimension by 0.97^d and
    the speakers by 2; T = I + N(0, 1 / L), psi sorted from U(0.05, 8), m = 0.1 N(0, 1)"""
    rng = np.random.RandomState(1000 * seed + 7 * n + L)
    scale = 0.97 ** np.arange(L)
    spk = 2.0 * rng.randn(K, L) * scale
    lab = np.arange(n) % K
    rng.shuffle(lab)
    z = (spk[lab] + rng.randn(n, L) * scale).astype(np.float32)
    T = np.eye(L) + rng.randn(L, L) / np.sqrt(L)
    psi = np.sort(rng.uniform(0.05, 8.0, L))[::-1].copy()
    m = 0.1 * rng.randn(L)
    return z, lab, (m, T, psi)


def conditions(ref, E):
    """the conditions of section 6p on a (longdouble) reference: the margins (energy, gap, floor), each must be met"""
    s, dim = ref["s"], ref["dim"]
    if ref["skip"]:
        return np.inf, np.inf, np.inf
    cum, tot = np.cumsum(s), s.sum()
    energy = float(np.abs(cum / tot - E).min())
    gap = float((s[dim - 1] - s[dim]) / s[0]) if dim < len(s) else np.inf
    return energy, gap, float(s[dim - 1] / s[0])


def assert_conditions(ref, E, what):
    energy, gap, floor = conditions(ref, E)
    assert energy >= 1e-5 and gap >= 1e-5 and floor >= 1e-6, (what, energy, gap, floor)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
class Yardstick:
    """the longdouble reference of one recording, its float64 twin and the bound M * e64 + floor per quantity"""

    def __init__(self, z, model, E, normalize_length=True, simple=False):
        self.z, self.E = z, E
        self.hi = pca_ref(z, model, E, LD, normalize_length, simple)
        self.lo = pca_ref(z, model, E, np.float64, normalize_length, simple)
        self.dim, self.skip = self.hi["dim"], self.hi["skip"]
        self.same_dim = self.lo["dim"] == self.dim
        self.e64, self.floor = {}, {}
        for name, hi, lo in self._quantities(self.lo["s"], self.lo["psi_r"], self.lo["S"] if self.same_dim else None):
            self.e64[name] = float(np.abs(hi - lo).max()) if lo is not None else 0.0
            self.floor[name] = 16 * ULP * float(np.abs(hi).max())

    def _quantities(self, s, psi_r, S):
        s1 = self.hi["s"][0] if self.hi["s"][0] > 0 else 1
        d = self.dim
        yield "s", self.hi["s"] / s1, None if s is None else np.asarray(s, dtype=LD) / s1
        yield "psi_r", self.hi["psi_r"], None if psi_r is None else np.asarray(psi_r, dtype=LD)[:d]
        yield "S", self.hi["S"], None if S is None else np.asarray(S, dtype=LD)

    def ratios(self, s, psi_r, S):
        """err / (e64 + floor) per quantity for a candidate (float64 arrays; psi_r may be zero padded)"""
        out = {}
        for name, hi, got in self._quantities(s, psi_r, S):
            err, den = float(np.abs(hi - got).max()), self.e64[name] + self.floor[name]
            out[name] = err / den if den > 0 else (0.0 if err == 0 else np.inf)
        return out

    def check(self, s, psi_r, S, what, M=M):
        out = self.ratios(s, psi_r, S)
        for name, hi, got in self._quantities(s, psi_r, S):
            err = float(np.abs(hi - got).max())
            assert err <= M * self.e64[name] + self.floor[name], (what, name, err, self.e64[name], self.floor[name])
        return out


def scores_fp64(U, psi_r, dim):
    """the fp64 score matrix of one recording from a back end's rows (zero padded to L), psi_r and dim, in numpy"""
    u, p = np.asarray(U, dtype=np.float64)[:, :dim], np.asarray(psi_r, dtype=np.float64)[:dim]
    g, k, K = dense_terms(p)
    q = -0.5 * (k[None, :] * u * u).sum(axis=1)
    return (u * g[None, :]) @ u.T + q[:, None] + q[None, :] + K
