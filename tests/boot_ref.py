"""Independent restatement of the speaker-level bootstrap for the tests: plain Python integers and one
division per rate, position by position; the counter-based hash of the counts table; and the literally replicated trial list."""
import math

M64 = (1 << 64) - 1


def mix(x):
    """SplitMix64's output function"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def counts_table(U, R, seed):
    rows = []
    for r in range(R):
        base = mix((mix(seed & M64) + r) & M64)
        row = [0] * U
        for j in range(U):
            h = mix((base + j) & M64)
            row[((h >> 32) * U) >> 32] += 1
        rows.append(row)
    return rows


def sorted_positions(scores):
    """stable, -0.0 equal to +0.0"""
    return sorted(range(len(scores)), key=lambda t: (scores[t] + 0.0, t))


def bayes_threshold(p, c_miss, c_fa):
    return math.log(c_fa * (1.0 - p)) - math.log(c_miss * p)


def replicate(scores, labels, ua, ub, c, costs, act_costs):
    """one replicate: {'flag', 'n_tar', 'n_non'} and, unless flagged, 'eer', 'eer_pos', 'min_dcf': [(value, pos)], 'act': [(value,
    miss, fa)]"""
    order = sorted_positions(scores)
    T = len(order)
    w = [c[ua[t]] if ua[t] == ub[t] else c[ua[t]] * c[ub[t]] for t in order]
    ct, cn, t_run, n_run = [], [], 0, 0
    for k, t in enumerate(order):
        if labels[t]:
            t_run += w[k]
        else:
            n_run += w[k]
        ct.append(t_run)
        cn.append(n_run)
    n_tar, n_non = ct[-1], cn[-1]
    out = {"flag": int(n_tar == 0 or n_non == 0), "n_tar": n_tar, "n_non": n_non}
    if out["flag"]:
        return out
    fnr = [ct[k] / float(n_tar) for k in range(T)]
    fpr = [1 - cn[k] / float(n_non) for k in range(T)]
    best = 0
    for k in range(1, T):
        if abs(fnr[k] - fpr[k]) < abs(fnr[best] - fpr[best]):
            best = k
    out["eer"], out["eer_pos"] = max(fpr[best], fnr[best]), best
    out["min_dcf"] = []
    for p, c_miss, c_fa in costs:
        cost = [c_miss * fnr[k] * p + c_fa * fpr[k] * (1 - p) for k in range(T)]
        j = 0
        for k in range(1, T):
            if cost[k] < cost[j]:
                j = k
        out["min_dcf"].append((cost[j] / min(c_miss * p, c_fa * (1 - p)), j))
    out["act"] = []
    for p, c_miss, c_fa in act_costs:
        eta = bayes_threshold(p, c_miss, c_fa)
        q = sum(1 for t in order if scores[t] < eta)
        miss = ct[q - 1] if q else 0
        fa = n_non - (cn[q - 1] if q else 0)
        f_miss, f_fa = miss / float(n_tar), fa / float(n_non)
        out["act"].append(((c_miss * f_miss * p + c_fa * f_fa * (1 - p)) / min(c_miss * p, c_fa * (1 - p)), miss, fa))
    return out


def replicated_list(scores, labels, ua, ub, c):
    """the trial list of the replicate written out: unit u becomes c[u] copies; a trial between different units exists for every pair
    of copies, a same-unit trial once per copy -> (scores, labels)"""
    s, lab = [], []
    for t in range(len(scores)):
        n = c[ua[t]] if ua[t] == ub[t] else c[ua[t]] * c[ub[t]]
        if ua[t] != ub[t]:
            n = sum(1 for _ in range(c[ua[t]]) for _ in range(c[ub[t]]))
        s += [scores[t]] * n
        lab += [labels[t]] * n
    return s, lab
