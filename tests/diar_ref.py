"""Independent restatement of the diarization back end, written from the rule's text and not from the product
code: the dense score expression in numpy.longdouble with its derived error bound, the average-linkage rule as a direct search over
all active pairs at every step (no cached minima), and the RTTM rule."""
import numpy as np

LD = np.longdouble


# ---- dense scores -----------------------------------------------------------------------------------------------------------------
def plda_terms(psi):
    """g_d = psi_d / (2 psi_d + 1), k_d = psi_d^2 / ((psi_d + 1)(2 psi_d + 1)), K = 0.5 sum_d (log(psi_d + 1) - log(1 + psi_d / (psi_d + 1)))"""
    psi = np.asarray(psi, dtype=np.float64)
    g = psi / (2 * psi + 1)
    k = psi ** 2 / ((psi + 1) * (2 * psi + 1))
    K = 0.5 * float(np.sum(np.log(psi + 1) - np.log(1 + psi / (psi + 1))))
    return g, k, K


def plda_q(U, k):
    return -0.5 * (np.asarray(k)[None, :] * U * U).sum(axis=1)


def dense_ref(U, q, g, K):
    """one recording: (r, bound) as float64 [n][n]; r = q_i + q_j + K + sum_d g_d U_id U_jd in longdouble, and
    bound = 2^-24 |r| + (D + 8) 2^-53 (|q_i| + |q_j| + |K| + sum_d |g_d U_id U_jd|): the rounding to float plus one fp64 rounding per
    term in any order"""
    U, q, g = np.asarray(U, dtype=LD), np.asarray(q, dtype=LD), np.asarray(g, dtype=LD)
    D = U.shape[1]
    r = (U * g) @ U.T + q[:, None] + q[None, :] + LD(K)
    mag = (np.abs(U) * np.abs(g)) @ np.abs(U).T + np.abs(q)[:, None] + np.abs(q)[None, :] + abs(LD(K))
    bound = LD(2.0) ** -24 * np.abs(r) + (D + 8) * LD(2.0) ** -53 * mag
    return r, bound, (D + 8) * LD(2.0) ** -53 * mag


def llr_direct(U, psi):
    """Plda::LogLikelihoodRatio(u_i, 1, u_j) for every pair, in the per-trial form spk_plda_llr states (fp64)"""
    psi = np.asarray(psi, dtype=np.float64)
    c, v = psi / (psi + 1), 1 + psi / (psi + 1)
    x, e = U[None, :, :], U[:, None, :]                                # out[i][j]: enrol i, test j
    d = x - c * e
    quad = (0.5 * (x * x / (psi + 1) - d * d / v)).sum(axis=2)
    return quad + 0.5 * (np.log(psi + 1).sum() - np.log(v).sum())


# ---- clustering -------------------------------------------------------------------------------------------------------------------
def ahc_ref(S, min_clusters=1, threshold=None):
    """S: float32 [n][n] (the upper triangle is read) -> (labels int32 [n], merges [(i, j)], costs [float64])"""
    S = np.asarray(S, dtype=np.float32)
    n = S.shape[0]
    C = np.zeros((n, n))
    iu = np.triu_indices(n, 1)
    C[iu] = -S[iu].astype(np.float64)
    C = C + C.T
    m = np.ones(n)
    active = np.ones(n, dtype=bool)
    member = [[w] for w in range(n)]
    merges, costs = [], []
    stop_at = max(min(int(min_clusters), n), 1)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    with np.errstate(all="ignore"):
        while active.sum() > stop_at:
            c = C / (m[:, None] * m[None, :])
            ok = upper & active[:, None] & active[None, :] & (c == c)
            c = np.where(ok, c, np.inf)
            flat = int(np.argmin(c))                                    # row-major: the smallest i, then the smallest j
            i, j = divmod(flat, n)
            best = c[i, j]
            if not best < np.inf:                                       # `c < best` from best = +inf: nothing was found
                break
            if threshold is not None and not best <= -float(threshold):
                break
            merges.append((i, j))
            costs.append(float(best))
            for k in range(n):
                if active[k] and k != i and k != j:
                    C[i, k] = C[i, k] + C[j, k]
                    C[k, i] = C[i, k]
            m[i] += m[j]
            active[j] = False
            member[i] += member[j]
            member[j] = []
    labels = np.zeros(n, dtype=np.int32)
    for lab, root in enumerate(sorted((min(g), a) for a, g in enumerate(member) if g), 1):
        labels[member[root[1]]] = lab
    return labels, merges, costs


def planted(n, k, seed, sep=6.0, dim=8):
    """tie-free planted-cluster data: points [n][dim], planted labels (1.. by lowest member), S = -euclidean distance (float32)"""
    rng = np.random.RandomState(seed)
    k = min(k, n)
    who = np.concatenate([np.arange(k), rng.randint(0, k, size=n - k)])
    rng.shuffle(who)
    centres = rng.randn(k, dim) * sep
    x = centres[who] + 0.3 * rng.randn(n, dim)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    first = {}
    for w, c in enumerate(who):
        first.setdefault(c, len(first) + 1)
    return x, np.array([first[c] for c in who], dtype=np.int32), (-d).astype(np.float32)


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


# ---- RTTM -------------------------------------------------------------------------------------------------------------------------
def rttm_ref(segments, labels, channel=0):
    """segments [(key, recording, start, end)], labels aligned with them -> lines"""
    order, per = [], {}
    for (key, reco, s, e), lab in zip(segments, labels):
        if reco not in per:
            per[reco] = []
            order.append(reco)
        per[reco].append({"s": float(s), "e": float(e), "l": int(lab)})
    out = []
    for reco in order:
        w = sorted(per[reco], key=lambda p: (p["s"], p["e"]))
        for a in range(len(w) - 1):
            cur, nxt = w[a], w[a + 1]
            if cur["l"] != nxt["l"] and nxt["s"] < cur["e"]:
                mid = (nxt["s"] + cur["e"]) / 2
                cur["e"] = mid
                nxt["s"] = mid
        merged = []
        for p in w:
            if merged and merged[-1]["l"] == p["l"] and p["s"] <= merged[-1]["e"]:
                merged[-1]["e"] = max(merged[-1]["e"], p["e"])
            else:
                merged.append(dict(p))
        for p in merged:
            if p["e"] - p["s"] > 0:
                out.append("SPEAKER %s %s %.3f %.3f <NA> <NA> %d <NA> <NA>" % (reco, channel, p["s"], p["e"] - p["s"], p["l"]))
    return out


def parse_rttm(lines):
    """-> recording -> [(start, duration, label)]"""
    out = {}
    for line in lines:
        f = line.split()
        assert len(f) == 10 and f[0] == "SPEAKER" and f[5] == f[6] == f[8] == f[9] == "<NA>", line
        out.setdefault(f[1], []).append((float(f[3]), float(f[4]), int(f[7])))
    return out
