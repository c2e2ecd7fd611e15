"""Shared by the CTC-loss tests: the float64 restatement of the loss and its torch-convention gradient, written
in numpy from the definition in include/rroi_align_hip.h section 15; the case table; the bound.

The bound is derived, not fitted.  Every log-domain quantity the evaluation meets (an lp, an alpha, a beta) is at most M in
magnitude, so one double operation on them errs by at most M * 2^-53; at most about 8 (T + 1) such operations lie on the
path to any output (per time step: a max, the differences from it, the exp of each -- whose errors the sum and the log
damp, their derivatives being <= 1 there --, the additions, the log, the addition of the max and of lp; one more step's
worth for the last lse), hence E = 8 (T + 1) M 2^-53 bounds the error of any alpha, beta, class sum or nll.
The loss: the kernel's nll and the restatement's each lie within E of the exact one, so they differ by at most 2 E before
the one rounding to float32.  The gradient: both exp arguments are <= 0 up to their error (lp is a log-probability; alpha
beta counts lp[k, t] twice, so the class sum plus nll minus lp is the log of the posterior of class k at step t), where
exp's derivative is <= 1, so an exp moves by no more than its argument does.  The first argument, lp, is exact.  The second is a class sum (E) plus the
nll (E) minus lp, each side: 2 E in the kernel and 2 E in the restatement.  So
    |grad - ref| <= ulp_out(ref) + 4 E        |nll - ref| <= ulp_fp32(ref) + 2 E
with ulp_out one unit in the last place of the output dtype at the reference value: a value evaluated in double and
rounded once can land one ulp from the rounded reference and no farther."""
import numpy as np
import torch

NINF = -np.inf
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def lse(vals):
    m = max(vals)
    if m == NINF:
        return NINF
    return m + np.log(sum(np.exp(v - m) for v in vals))


def lse_rows(v):
    """log of the sum of exp over axis 0 of v (terms in ascending row order); -inf where every term is."""
    m = v.max(0)
    safe = np.where(m == NINF, 0.0, m)
    with np.errstate(divide="ignore"):
        return np.where(m == NINF, NINF, safe + np.log(np.exp(v - safe).sum(0)))


def feasible_structure(target, L, Tn, T, K, width):
    return 0 <= Tn <= T and 0 <= L <= min(width, T) and all(0 <= int(c) < K for c in target[:max(L, 0)])


def ref64(lp, targets, in_len, tgt_len, blank=0, zero_infinity=False):
    """lp (T, N, K) float64 array; targets (N, width) ints; lengths of N.  -> nll (N) float64, grad (T, N, K) float64 (for
    grad_output = 1), M: the largest finite |alpha|, |beta| or |lp| met (1 at least)."""
    lp = np.asarray(lp, dtype=np.float64)
    T, N, K = lp.shape
    targets = np.asarray(targets).reshape(N, -1)
    nll, grad, M = np.zeros(N), np.zeros((T, N, K)), 1.0
    fin = np.abs(lp[np.isfinite(lp)])
    if fin.size:
        M = max(M, float(fin.max()))
    for n in range(N):
        Tn, L = int(in_len[n]), int(tgt_len[n])
        if not feasible_structure(targets[n], L, Tn, T, K, targets.shape[1]):
            nll[n] = 0.0 if zero_infinity else np.inf
            continue
        ext = [blank] * (2 * L + 1)
        ext[1::2] = [int(c) for c in targets[n, :L]]
        S = len(ext)
        if Tn == 0:
            nll[n] = 0.0 if L == 0 or zero_infinity else np.inf
            continue
        ext = np.array(ext)
        odd = ext != blank
        skip_a = np.zeros(S, dtype=bool)          # s may come from s - 2
        skip_a[2:] = odd[2:] & (ext[2:] != ext[:-2])
        skip_b = np.zeros(S, dtype=bool)          # s may go to s + 2
        skip_b[:-2] = odd[:-2] & (ext[:-2] != ext[2:])
        row = lp[:Tn, n, :][:, ext]               # (Tn, S): lp[l'_s, t]
        a = np.full((Tn, S), NINF)
        b = np.full((Tn, S), NINF)
        a[0, :2] = row[0, :2]
        for t in range(1, Tn):
            p = a[t - 1]
            p1 = np.concatenate(([NINF], p[:-1]))
            p2 = np.where(skip_a, np.concatenate(([NINF, NINF], p[:-2]))[:S], NINF)
            a[t] = row[t] + lse_rows(np.stack([p, p1, p2]))
        b[Tn - 1, max(S - 2, 0):] = row[Tn - 1, max(S - 2, 0):]
        for t in range(Tn - 2, -1, -1):
            p = b[t + 1]
            p1 = np.concatenate((p[1:], [NINF]))
            p2 = np.where(skip_b, np.concatenate((p[2:], [NINF, NINF]))[:S], NINF)
            b[t] = row[t] + lse_rows(np.stack([p, p1, p2]))
        for arr in (a, b):
            f = np.abs(arr[np.isfinite(arr)])
            if f.size:
                M = max(M, float(f.max()))
        ll = lse(list(a[Tn - 1, max(S - 2, 0):]))
        if ll == NINF:
            nll[n] = 0.0 if zero_infinity else np.inf
            continue                                    # an infinite loss: the gradient is defined as 0
        nll[n] = -ll
        x = lp[:Tn, n, :]
        g = np.where(x == NINF, 0.0, np.exp(x))         # classes outside the target: the class sum is empty
        ab = a + b
        for k in sorted(set(ext.tolist())):
            cls = lse_rows(ab[:, ext == k].T)           # (Tn,): over the positions of class k, ascending
            with np.errstate(invalid="ignore"):
                sub = np.where((cls == NINF) | (x[:, k] == NINF), 0.0, np.exp(cls + nll[n] - x[:, k]))
            g[:, k] -= sub
        grad[:Tn, n, :] = g
    return nll, grad, M


def E_of(T, M):
    return 8.0 * (T + 1) * M * 2.0 ** -53


def ulp(ref, dtype):
    """One unit in the last place of `dtype` at each |ref| (float64 array): the spacing of the binade |ref| lies in, the
    subnormal spacing below the smallest normal."""
    p, emin = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    e = np.floor(np.log2(np.where(ref > 0, ref, 1.0)))
    e = np.where(ref > 0, np.maximum(e, emin), emin)
    return 2.0 ** (e - (p - 1))


def grad_ratio(got, ref, dtype, T, M, scale=1.0, extra=0.0):
    """max over elements of |got - ref| / (ulp_out(ref) + 4 E * scale + extra); got: a tensor or array, ref float64."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    tol = ulp(ref, dtype) + 4.0 * E_of(T, M) * scale + extra
    return float((np.abs(got - ref) / tol).max()) if ref.size else 0.0


def nll_ratio(got, ref, T, M):
    """Likewise for the losses, |got - ref| <= ulp_fp32(ref) + 2 E; an infinite reference must be met exactly."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    inf = ~np.isfinite(ref)
    if (got[inf] != ref[inf]).any() or not np.isfinite(got[~inf]).all():
        return float("inf")
    if not (~inf).any():
        return 0.0
    r = ref[~inf]
    return float((np.abs(got[~inf] - r) / (ulp(r, torch.float32) + 2.0 * E_of(T, M))).max())


def log_probs(T, N, K, seed, kind="random", targets=None, tgt_len=None, blank=0):
    """float32 log-probabilities (T, N, K) as a torch tensor, normalised in double before the rounding.
    random: log_softmax of N(0, 2) logits.  certain: the mass on a valid alignment of each target (each label then a blank,
    blanks to the end), every other class 30 nats below: nll ~ 0, the gradient a difference of nearly equal numbers.
    holes: random with a tenth of the entries -inf, none of them a blank's."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((T, N, K)) * 2.0
    if kind == "certain":
        z = rng.standard_normal((T, N, K)) * 0.1
        for n in range(N):
            path = []
            for c in targets[n][:tgt_len[n]]:
                path += [int(c), blank]
            path = (path + [blank] * T)[:T]
            for t in range(T):
                z[t, n, path[t]] += 30.0
    z = z - z.max(2, keepdims=True)
    lp = z - np.log(np.exp(z).sum(2, keepdims=True))
    if kind == "holes":
        hole = rng.random((T, N, K)) < 0.1
        hole[:, :, blank] = False
        lp = np.where(hole, NINF, lp)
    return torch.from_numpy(lp.astype(np.float32))


def _targets(rng, N, K, blank, lens, width):
    labels = [k for k in range(K) if k != blank]
    tg = np.zeros((N, width), dtype=np.int64)
    for n, L in enumerate(lens):
        tg[n, :L] = rng.choice(labels, L)
    return tg


def _case(name, T, N, K, blank, lens, in_len, kind="random", width=None, seed=0, edit=None):
    """A case: dict(name, T, N, K, blank, targets (N, width) int64 array, tgt_len, in_len, kind, seed)."""
    width = max([1] + [L for L in lens if L <= T]) if width is None else width
    rng = np.random.default_rng(1000 + seed)
    tg = _targets(rng, N, K, blank, [min(max(L, 0), width) for L in lens], width)
    c = dict(name=name, T=T, N=N, K=K, blank=blank, targets=tg, tgt_len=list(lens), in_len=list(in_len), kind=kind, seed=seed)
    if edit:
        edit(c)
    return c


def _repeat(c):          # sequence 0: one character repeated; 1: exactly feasible; 2: one step short of feasible
    c["targets"][0, :c["tgt_len"][0]] = c["targets"][0, 0]
    for n in (1, 2):
        L = c["tgt_len"][n]
        reps = int((c["targets"][n, 1:L] == c["targets"][n, :L - 1]).sum())
        c["in_len"][n] = L + reps - (n == 2)


def _pairs(c):           # repeats next to each other and apart: a a b a, so that the class chains have gaps
    for n in range(c["N"]):
        L = c["tgt_len"][n]
        if L >= 4:
            a = c["targets"][n, 0]
            c["targets"][n, 1] = a
            c["targets"][n, 3] = a


def _bad_label(c):
    c["targets"][1, 1] = c["K"]
    c["targets"][2, 0] = -1


# The smallest cases at which each mechanism can fail (T: 1, 2, 33 -- more than two chunks of 16, a ragged last one --, 96,
# 160; S: 1, 3, 63 and 65 -- one wave of positions and one more --, 129; K: 2, 5, 87, 130 -- the last halves the chunk --;
# N: 1, 3, 32; both blanks; ragged, full, 1 and 0 input lengths; repeats; near-certain inputs; -inf entries; infeasible
# sequences).  K = 130 with L = 64 at T = 160 keeps its alpha rows in the workspace; every other case in LDS.
CASES = [
    _case("t1", 1, 3, 5, 0, [0, 1, 1], [1, 1, 0]),
    _case("t2_k2", 2, 3, 2, 0, [1, 2, 0], [2, 2, 1], edit=lambda c: c["targets"].__setitem__((1, slice(None)), [1, 1])),
    _case("t33_ragged", 33, 3, 5, 4, [4, 9, 0], [33, 20, 1], edit=_pairs),
    _case("t96_train", 96, 32, 87, 0, [3 + i % 7 for i in range(32)], [96] * 32, seed=1),
    _case("l31_l32", 96, 3, 87, 86, [31, 32, 1], [96, 80, 96], seed=2),
    _case("l64_ws", 160, 3, 130, 0, [64, 40, 5], [160, 130, 160], seed=3, edit=_pairs),
    _case("n1_l16", 33, 1, 5, 0, [16], [33], seed=4),
    _case("repeats", 33, 3, 5, 0, [6, 8, 8], [33, 0, 0], seed=5, edit=_repeat),
    _case("certain", 33, 3, 87, 0, [5, 9, 2], [33, 30, 12], kind="certain", seed=6),
    _case("holes", 33, 3, 5, 2, [3, 5, 0], [33, 25, 7], kind="holes", seed=7),
    _case("bad_label", 33, 3, 5, 0, [3, 4, 2], [33, 33, 33], seed=8, edit=_bad_label),
    _case("bad_lengths", 33, 3, 5, 0, [3, 7, 2], [33, 33, 34], width=4, seed=9),
]
FINITE_FEASIBLE = ("t33_ragged", "t96_train", "l31_l32", "l64_ws", "n1_l16", "certain")
CASE = {c["name"]: c for c in CASES}

_cache = {}


def materialise(case, dtype=torch.float32):
    """(lp: the case's log-probabilities rounded to dtype, a CPU tensor; ref: ref64 on exactly those values), computed once
    per (case, dtype) and shared: treat both as read-only."""
    key = (case["name"], dtype)
    if key not in _cache:
        lp = log_probs(case["T"], case["N"], case["K"], case["seed"], case["kind"], case["targets"],
                       [min(max(L, 0), case["targets"].shape[1]) for L in case["tgt_len"]], case["blank"]).to(dtype)
        _cache[key] = (lp, ref64(lp.double().numpy(), case["targets"], case["in_len"], case["tgt_len"], case["blank"]))
    return _cache[key]
