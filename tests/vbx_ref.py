"""Independent restatement of VBx, written from the rule's text and not from the product code: the full S x S
transition matrix, a plain log-sum-exp with the maximum taken out, the dtype a parameter (numpy.longdouble is the yardstick, float64
gives the yardstick's own error), the tolerance rule of section 6o and the planted-data generator the tests share."""
import numpy as np

LD = np.longdouble
FLOOR = 2.0 ** -49              # 16 ulp of 1: the floor for gamma and pi; for the ELBO it is relative
M_FACTOR = 4                    # M of the tolerance rule: the next power of two at least 4 times the largest ratio err / (e64 + floor)
#                                 measured on the GPU (0.54, the ELBO of a one-iteration run; DESIGN.md section 6o lists them)
M_CEILING = 64                  # the largest M the rule allows: what two float64 runs of different forms are held to against each other
CASES = [(1, 4, 2, 1), (2, 3, 3, 2), (65, 5, 4, 3), (130, 128, 7, 3), (257, 150, 16, 4), (300, 128, 10, 4)]     # (T, D, S, K)
PARAMS = [(0.3, 17.0, 0.99), (1.0, 1.0, 0.9)]                                                                # (Fa, Fb, loopP)


def lse(a, axis):
    """log sum exp along `axis` with the maximum taken out; -inf where every term is -inf"""
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def vbx_ref(X, Phi, gamma, pi, Fa, Fb, loopP, max_iters, epsilon, dtype=LD, linear=False):
    """One recording -> (gamma [T][S], pi [S], elbo list) in `dtype`.  linear: the O(S) form of the two recursions that the rule
    allows (the rows of tr differ only on the diagonal) in place of the S x S form."""
    X, Phi, gamma, pi = (np.array(v, dtype=dtype) for v in (X, Phi, gamma, pi))
    Fa, Fb, loopP, half, one = dtype(Fa), dtype(Fb), dtype(loopP), dtype(0.5), dtype(1)
    T, D = X.shape
    S = gamma.shape[1]
    rho = X * np.sqrt(Phi)[None, :]
    G = -half * ((X * X).sum(axis=1) + D * np.log(dtype(8) * np.arctan(one)))
    elbo = []
    with np.errstate(divide="ignore", under="ignore"):
        for it in range(max_iters):
            N = gamma.sum(axis=0)
            invL = one / (one + (Fa / Fb) * N[:, None] * Phi[None, :])
            alpha = (Fa / Fb) * invL * (gamma.T @ rho)
            logp = Fa * (rho @ alpha.T - half * ((invL + alpha ** 2) @ Phi)[None, :] + G[:, None])
            ltr = np.log(loopP * np.eye(S, dtype=dtype) + (one - loopP) * pi[None, :])
            lfw = np.empty((T, S), dtype=dtype)
            lbw = np.zeros((T, S), dtype=dtype)
            lfw[0] = logp[0] + np.log(pi)
            for t in range(1, T):
                if linear:
                    m = lfw[t - 1].max()
                    e = np.exp(lfw[t - 1] - m)
                    lfw[t] = logp[t] + m + np.log(loopP * e + (one - loopP) * pi * e.sum())
                else:
                    lfw[t] = logp[t] + lse(lfw[t - 1][:, None] + ltr, 0)
            for t in range(T - 2, -1, -1):
                v = logp[t + 1] + lbw[t + 1]
                if linear:
                    m = v.max()
                    e = np.exp(v - m)
                    lbw[t] = m + np.log(loopP * e + (one - loopP) * (pi * e).sum())
                else:
                    lbw[t] = lse(ltr + v[None, :], 1)
            tll = lse(lfw[T - 1], 0)
            gamma = np.exp(lfw + lbw - tll)
            elbo.append(tll + half * Fb * (np.log(invL) - invL - alpha ** 2 + one).sum())
            if T > 1:
                pi = gamma[0] + (one - loopP) * pi * np.exp(lse(lfw[:-1], 1)[:, None] + logp[1:] + lbw[1:] - tll).sum(axis=0)
            else:
                pi = gamma[0].copy()
            pi = pi / pi.sum()
            if it > 0 and elbo[-1] - elbo[-2] < epsilon:
                break
    return gamma, pi, elbo


def init_gamma(labels, S, smoothing=7.0):
    """gamma_ts = softmax_s(smoothing [label_t == s]) over S states; labels from 0"""
    z = smoothing * (np.asarray(labels)[:, None] == np.arange(S)[None, :])
    e = np.exp(z)
    return e / e.sum(axis=1, keepdims=True)


def planted(T, D, S, K, seed, Phi=None):
    """-> (X [T][D], Phi [D], truth [T] in 0 .. K - 1, first [T] in 0 .. S - 1): Phi from a gamma distribution, K speaker means drawn
    N(0, diag(Phi)), runs of eight windows per speaker (the first K runs name every speaker once) with unit noise, and first-pass
    labels that are the truth with 30 % of the windows reassigned at random over the S states.  Phi: use these variances instead (the
    recordings of one batch share them)"""
    rng = np.random.RandomState(seed)
    drawn = rng.gamma(2.0, 2.0, size=D)
    Phi = drawn if Phi is None else np.asarray(Phi, dtype=np.float64)
    means = rng.randn(K, D) * np.sqrt(Phi)[None, :]
    runs = (T + 7) // 8
    who = np.concatenate([np.arange(K), rng.randint(0, K, size=max(runs - K, 0))])[:runs]
    truth = np.repeat(who, 8)[:T]
    X = means[truth] + rng.randn(T, D)
    first = truth.copy()
    move = rng.rand(T) < 0.3
    first[move] = rng.randint(0, S, size=int(move.sum()))
    return X, Phi, truth, first


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def labels_of(gamma):
    """argmax_s with ties to the lowest s, renumbered 1, 2, ... by lowest member window"""
    a = np.argmax(np.asarray(gamma, dtype=np.float64), axis=1)
    seen = {}
    return np.array([seen.setdefault(int(s), len(seen) + 1) for s in a], dtype=np.int32)


def top_two_gap(gamma):
    """the smallest difference between the largest and the second largest gamma of a window (1 for a single state)"""
    g = np.sort(np.asarray(gamma, dtype=np.float64), axis=1)
    return 1.0 if g.shape[1] < 2 else float((g[:, -1] - g[:, -2]).min())


class Yardstick:
    """The longdouble run of one input with the error of the float64 run of the same restatement against it: for each of gamma, pi
    and the ELBO (relative) the bound is M_FACTOR * e64 + FLOOR.  Computed once per input and shared."""

    def __init__(self, X, Phi, gamma, pi, Fa, Fb, loopP, max_iters, epsilon):
        self.gamma, self.pi, self.elbo = vbx_ref(X, Phi, gamma, pi, Fa, Fb, loopP, max_iters, epsilon, LD)
        g64, p64, e64 = vbx_ref(X, Phi, gamma, pi, Fa, Fb, loopP, max_iters, epsilon, np.float64)
        self.n_iters = len(self.elbo)
        self.same_length = len(e64) == self.n_iters
        n = min(len(e64), self.n_iters)
        self.elbo = np.array(self.elbo, dtype=LD)
        self.e64 = {"gamma": float(np.abs(g64.astype(LD) - self.gamma).max()), "pi": float(np.abs(p64.astype(LD) - self.pi).max()),
                    "elbo": float((np.abs(np.array(e64[:n], dtype=LD) - self.elbo[:n]) / np.abs(self.elbo[:n])).max())}
        self.bound = {k: M_FACTOR * v + FLOOR for k, v in self.e64.items()}

    def errors(self, gamma, pi, elbo):
        """the errors of a result against the longdouble run: gamma and pi absolute, the ELBO relative"""
        e = np.asarray(elbo, dtype=np.float64)[:self.n_iters].astype(LD)
        return {"gamma": float(np.abs(np.asarray(gamma, dtype=np.float64).astype(LD) - self.gamma).max()),
                "pi": float(np.abs(np.asarray(pi, dtype=np.float64).astype(LD) - self.pi).max()),
                "elbo": float((np.abs(e - self.elbo) / np.abs(self.elbo)).max())}

    def ratios(self, gamma, pi, elbo):
        """err / (e64 + FLOOR) per quantity: what section 6o quotes and M_FACTOR is chosen from"""
        err = self.errors(gamma, pi, elbo)
        return {k: err[k] / (self.e64[k] + FLOOR) for k in err}

    def check(self, gamma, pi, elbo, what="", M=None):
        err = self.errors(gamma, pi, elbo)
        bound = self.bound if M is None else {k: M * v + FLOOR for k, v in self.e64.items()}
        for k in ("gamma", "pi", "elbo"):
            print("vbx %s %s: error %.3e, yardstick %.3e, bound %.3e, ratio %.2f" % (what, k, err[k], self.e64[k], bound[k],
                                                                                    err[k] / (self.e64[k] + FLOOR)))
        for k in ("gamma", "pi", "elbo"):
            assert err[k] <= bound[k], (what, k, err[k], bound[k])


_PLANTED = {}


def planted_case(T, D, S, K, Fa, Fb, loopP, iters=10):
    """the planted input of one (case, parameter) pair with its yardstick, made once: dict(X, Phi, truth, first, gamma0, pi0, y)"""
    key = (T, D, S, K, Fa, Fb, loopP, iters)
    if key not in _PLANTED:
        X, Phi, truth, first = planted(T, D, S, K, seed=1000 * T + D)
        g0, p0 = init_gamma(first, S), np.full(S, 1.0 / S)
        _PLANTED[key] = {"X": X, "Phi": Phi, "truth": truth, "first": first, "gamma0": g0, "pi0": p0,
                         "y": Yardstick(X, Phi, g0, p0, Fa, Fb, loopP, iters, -np.inf)}
    return _PLANTED[key]


# early stopping: planted recordings (T, S, K, seed) at D = 8 with shared variances whose ELBO steps, up to the stop, all lie outside
# [eps / 100, 100 eps] (tests/test_vbx_cpu.py asserts it on the reference), and which stop after different iterations
EARLY = {"epsilon": 1e-5, "max_iters": 12, "Fa": 0.3, "Fb": 17.0, "loopP": 0.99, "D": 8,
         "cases": [(40, 4, 2, 3), (50, 3, 2, 1), (33, 4, 3, 3), (24, 3, 2, 5)]}
_EARLY = []


def early_cases():
    """-> [dict(X, Phi, gamma0, pi0, y (the yardstick of the run stopped by EARLY's epsilon), elbo (y's))], made once; one Phi for all"""
    if not _EARLY:
        Phi = planted(1, EARLY["D"], 4, 2, 0)[1]
        for T, S, K, seed in EARLY["cases"]:
            X, _, _, first = planted(T, EARLY["D"], S, K, seed, Phi)
            g0, p0 = init_gamma(first, S), np.full(S, 1.0 / S)
            y = Yardstick(X, Phi, g0, p0, EARLY["Fa"], EARLY["Fb"], EARLY["loopP"], EARLY["max_iters"], EARLY["epsilon"])
            _EARLY.append({"X": X, "Phi": Phi, "gamma0": g0, "pi0": p0, "y": y, "elbo": y.elbo})
    return _EARLY
