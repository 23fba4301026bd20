"""Elite selection + refit + final pick (refit_plan, tdmpc2_amd/csrc/common.cuh; tdmpc2/tdmpc2.py:184-206) in numpy fp64 on the
kernel's own fp32 input bits, the gates its fp32 outputs are held to, a port of the kernel's branch decisions, and the crafted
cases.  tests/test_refit_edges.py proves all of it on the CPU; tests/test_gpu_refit_edges.py holds the kernel to it.

Selection is exact: after nan_to_num (NaN -> 0, +-inf -> +-FLT_MAX) and with -0 folded into +0, a stable sort on
(-value, index), padding rows (index >= Nvalid) behind every real row.  That is the project's contract "value descending, index
ascending on ties" (DESIGN 3.3).

Gates: first-order bounds from counted roundings (u = 2^-24), times MARGIN for the second-order terms.
  value, elite_idx (order included), prev_mean against the last mean: bit-exact.
  score s_k = e_k / S, e_k = exp(arg_k), arg_k = tau (v_k - v_max):
      r_k = 2 u |arg_k| (two roundings of arg, pushed through exp) + 2 EXPF_ULP 2^-23 (expf, twice its measured worst error)
      relative gate  r_k + sum_j s_j r_j (the same errors inside S) + (K + 2) u (the K - 1 additions of S, the division, and the
      second sum the kernel forms for the mean), absolute floor FLT_MIN (a flushed denormal score is not a failure).
  mean m = sum s a / (sum s + 1e-9):  u (2 K + 4) sum |s a| / sum s   (products, the additions of both sums, the division, the
      1e-9 that fp32 drops)  +  sum ds_k |a_k - m| / sum s   with ds_k the score gate.
  variance s2 = sum s d^2 / (sum s + 1e-9), d = a - m:  u (2 K + 6) s2  +  sum s 2 |d| dm / sum s + dm^2  (dm: the mean gate)
      +  sum ds_k |d_k^2 - s2| / sum s.  std must lie in [clamp(sqrt(max(s2 - g, 0))), clamp(sqrt(s2 + g))], widened by two
      roundings (the division and the square root), then multiplied by the mask: no case needs excluding at a clamp.
  action = clamp(a + std0 eps): 2^-23 (|a| + |std0 eps|) around the fp64 value from the GPU's OWN std[0] bits; the clamp is exact.
  Gumbel pick: argmax of log s_k - log ex_k; it must equal the fp64 pick whenever the fp64 top two are further apart than the
      two logits' gates: the score gate + 3 ulp for each logf (the OpenCL bound) + the addition + the softmax stage behind it
      (a subtraction, expf, a division).  On an exact tie the first elite wins.
"""
import numpy as np

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
MARGIN = 2.0
# the worst error of the device's expf against fp64 on [-104, 0], in ulp: what tests/test_gpu_refit_edges.py measured on the
# MI355X (profiles/refit_edges.json: "expf_ulp"); that test fails if the device ever shows more.  The score gate takes twice it.
EXPF_ULP = 0.84
LOGF_ULP = 3.0


# ------------------------------------------------------------------ the kernel's branch decisions (common.cuh, plan_run.hip)
def sort_width(N):
    M = 64
    while M < N:
        M <<= 1
    return M


def refit_threads(N):
    """Threads of a k_refit workgroup: the sort width."""
    return sort_width(N)


def refit_lds_bytes(N, K, H, A, budget=48 * 1024):
    """(dynamic LDS bytes, staged) as refit_lds_bytes in common.cuh."""
    base = (2 * sort_width(N) + 3 * K + 4 * H * A + 48) * 4 + 64
    elite = K * H * A * 4
    staged = base + elite <= budget
    return (base + elite if staged else base), staged


ROLLOUT_THREADS = 512  # ks_rollout / ks_rollout_cl / ks_rollout_cl2: 8 wavefronts


def fold_budget(A):
    """LDS the in-launch refit may use: the 32-row tile of the fused family (row = [z | a padded to 16] + 4 floats, either arithmetic)."""
    apad = (A + 15) // 16 * 16
    return 32 * (4 * (512 + apad) + 16)


def branches(N, K, H, A, in_launch=False):
    """Which paths refit_plan takes: `sorted` (bitonic sort, one key per thread) or counting; `staged` (elite actions in LDS: quad
    sums) or unstaged (serial loop over global memory); `in_launch` only when the elites fit the tile budget (else k_refit)."""
    if in_launch:
        _, staged = refit_lds_bytes(N, K, H, A, fold_budget(A))
        if staged:
            return dict(sorted=sort_width(N) <= ROLLOUT_THREADS, staged=True, in_launch=True)
    _, staged = refit_lds_bytes(N, K, H, A)
    return dict(sorted=True, staged=staged, in_launch=False)


# ------------------------------------------------------------------ the reference
def nan_to_num(value):
    v = np.asarray(value, np.float32).copy()
    v[np.isnan(v)] = 0.0
    v[v == np.inf] = np.float32(FLT_MAX)
    v[v == -np.inf] = np.float32(-FLT_MAX)
    return v


def select(v, K, Nvalid=None, mut=None):
    """Elite indices [K]: stable sort on (-value, index), -0 == +0, padding rows last."""
    N = len(v)
    NV = N if not Nvalid else Nvalid
    key = v.astype(np.float64) + 0.0
    idx = np.arange(N)
    third = np.zeros(N)
    if mut == "negzero_below":
        third = np.signbit(v).astype(np.float64) * (v == 0)
    tie = -idx if mut == "tie_reversed" else idx
    pad = np.zeros(N) if mut == "padding_eligible" else (idx >= NV).astype(np.float64)
    order = np.lexsort((tie, third, -key, pad))
    return order[:K].astype(np.int32)


def refit_ref(value, actions, K, temperature, min_std, max_std, Nvalid=None, mask=None, gumbel_exp=None, final_eps=None,
              eval_mode=False, last=False, mut=None, expf_ulp=None):
    """value [N] fp32 bits, actions [H, N, A] fp32 bits -> everything refit_plan writes, in fp64, and the gates (module docstring).
    `mut`: one of MUTATIONS, a mistake made on purpose (tests/test_refit_edges.py)."""
    value = np.asarray(value, np.float32)
    acts = np.asarray(actions, np.float32).astype(np.float64)
    H, N, A = acts.shape
    tau = float(np.float32(temperature))
    lo_c, hi_c = float(np.float32(min_std)), float(np.float32(max_std))
    xu = 2.0 * (EXPF_ULP if expf_ulp is None else expf_ulp) * 2.0 ** -23
    v32 = value.copy() if mut == "inf_kept" else nan_to_num(value)
    if mut == "inf_kept":
        v32[np.isnan(v32)] = 0.0
    ei = select(v32, K, Nvalid, mut)
    ev = v32[ei].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        arg = tau * (ev - ev[0])
        e = np.exp(arg)
        S = e.sum()
        s = e if mut == "single_normalisation" else e / S
        r = 2.0 * U * np.abs(arg) + xu
        r = np.where(e > 0, r, 0.0)  # a score that is 0 in fp64 has no relative error to speak of: the floor covers it
        g_rel = MARGIN * (r + float((e / S * r).sum()) + (K + 2) * U)
        ds = np.where(s > 0, s * g_rel, 0.0) + FLT_MIN
        w = s.copy()
        if mut == "last_elites_dropped":
            w[K & ~3:] = 0.0
        ssum = s.sum()
        den = ssum + 1e-9
        ea = acts[:, ei, :]  # [H, K, A]
        wk = w[None, :, None]
        m = (wk * ea).sum(1) / den
        g_m = MARGIN * (U * (2 * K + 4) * (np.abs(s[None, :, None] * ea)).sum(1) / ssum
                        + (ds[None, :, None] * np.abs(ea - m[:, None, :])).sum(1) / ssum)
        d = ea - m[:, None, :]
        s2 = (wk * d * d).sum(1) / den
        if mut == "unbiased_variance":
            s2 = s2 * K / max(K - 1, 1)
        g_v = MARGIN * (U * (2 * K + 6) * s2 + (s[None, :, None] * 2.0 * np.abs(d)).sum(1) / ssum * g_m + g_m * g_m
                        + (ds[None, :, None] * np.abs(d * d - s2[:, None, :])).sum(1) / ssum)
    mk = np.ones(A) if mask is None else np.asarray(mask, np.float64).reshape(A)
    clamp = lambda x: np.minimum(np.maximum(x, lo_c), hi_c)
    if mut == "clamp_after_mask":
        std = clamp(np.sqrt(s2) * mk)
    else:
        std = clamp(np.sqrt(s2)) * mk
    std_lo = clamp(np.sqrt(np.maximum(s2 - g_v, 0.0))) * (1.0 - 2.0 ** -23) * mk
    std_hi = clamp(np.sqrt(s2 + g_v)) * (1.0 + 2.0 ** -23) * mk
    out = dict(value=v32, elite_idx=ei, score=s, g_score=ds, mean=m * mk, g_mean=g_m * mk, std=std, std_lo=std_lo, std_hi=std_hi,
               var=s2, staged_rows=ea)
    if not last:
        return out
    ex = np.asarray(gumbel_exp, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        logit = np.log(s) - np.log(ex)
        g_logit = MARGIN * (np.where(s > 0, g_rel, 0.0) + LOGF_ULP * 2.0 ** -23 * (np.abs(np.log(s)) + np.abs(np.log(ex)))
                            + 2.0 ** -23 * np.abs(logit) + xu + 4 * U)
    order = np.lexsort((np.arange(K), -logit))
    top = int(order[0])
    if K > 1:
        second = int(order[1])
        margin = float(logit[top] - logit[second])
        gate = float(g_logit[top] + (g_logit[second] if np.isfinite(logit[second]) else 0.0))
        # equal scores and equal exponentials give identical bits on the device too: a tie by construction
        tied = bool(s[top] == s[second] and ex[top] == ex[second])
    else:
        margin, gate, tied = np.inf, 0.0, False
    out.update(pick=top, pick_margin=margin, pick_gate=gate, pick_tied=tied, logit=logit)
    t_pick = 1 if (mut == "pick_from_step_1" and H > 1) else 0
    out["pick_action"] = acts[t_pick, ei[top], :]
    out["final_eps"] = None if eval_mode else np.asarray(final_eps, np.float32).astype(np.float64)
    return out


MUTATIONS = ("tie_reversed", "negzero_below", "inf_kept", "padding_eligible", "last_elites_dropped", "unbiased_variance",
             "clamp_after_mask", "single_normalisation", "pick_from_step_1")


def action_of(ref, std0):
    """(action in fp64 from the given std[0] bits, its gate, the unfused fp32 expression, the fused one)."""
    a = ref["pick_action"]
    if ref["final_eps"] is None:
        x = a.copy()
        return np.clip(x, -1.0, 1.0), np.zeros_like(x), np.clip(x, -1, 1).astype(np.float32), np.clip(x, -1, 1).astype(np.float32)
    sd, eps = np.asarray(std0, np.float32).astype(np.float64), ref["final_eps"]
    x = a + sd * eps
    gate = 2.0 ** -23 * (np.abs(a) + np.abs(sd * eps))
    a32, sd32, eps32 = a.astype(np.float32), sd.astype(np.float32), eps.astype(np.float32)
    unfused = np.clip(a32 + sd32 * eps32, np.float32(-1), np.float32(1))
    fused = np.clip(x, -1.0, 1.0).astype(np.float32)  # a + sd eps is exact in fp64 up to its one rounding
    return np.clip(x, -1.0, 1.0), gate, unfused, fused


def as_got(ref):
    """A reference result (a mutated one, or another arithmetic's) in the shape of the kernel's fp32 outputs."""
    with np.errstate(over="ignore", invalid="ignore"):
        got = {k: np.asarray(ref[k]).astype(np.float32) for k in ("value", "score", "mean", "std")}
    got["elite_idx"] = ref["elite_idx"]
    if "pick" in ref:
        x = ref["pick_action"] if ref["final_eps"] is None else ref["pick_action"] + got["std"][0].astype(np.float64) * ref["final_eps"]
        got["action"] = np.clip(x, -1.0, 1.0).astype(np.float32)
        got["prev_mean"] = got["mean"]
    return got


def _ratio(err, gate):
    err, gate = np.asarray(err, np.float64), np.asarray(gate, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / np.maximum(gate, 1e-300))
    q = np.where(np.isnan(q), np.inf, q)
    return float(np.max(q)) if q.size else 0.0


def check(ref, got):
    """err / gate per quantity of `got` (fp32 arrays named as the kernel's outputs; missing ones are skipped) against
    refit_ref's result.  Bit-exact quantities give 0 or inf."""
    out = {}
    if "value" in got:
        out["value"] = 0.0 if np.array_equal(np.asarray(got["value"], np.float32).view(np.uint32), ref["value"].view(np.uint32)) else np.inf
    out["elite_idx"] = 0.0 if np.array_equal(np.asarray(got["elite_idx"]).astype(np.int64), ref["elite_idx"].astype(np.int64)) else np.inf
    sc = np.asarray(got["score"], np.float64)
    out["score"] = _ratio(np.abs(sc - ref["score"]), ref["g_score"]) if np.isfinite(sc).all() else np.inf
    mean = np.asarray(got["mean"], np.float64)
    out["mean"] = _ratio(np.abs(mean - ref["mean"]), ref["g_mean"]) if np.isfinite(mean).all() else np.inf
    std = np.asarray(got["std"], np.float64)
    if np.isfinite(std).all():
        mid, half = (ref["std_hi"] + ref["std_lo"]) / 2, (ref["std_hi"] - ref["std_lo"]) / 2
        out["std"] = _ratio(np.abs(std - mid), half)
    else:
        out["std"] = np.inf
    if "pick" in ref and "action" in got:
        a = np.asarray(got["action"], np.float32)
        want, gate, unfused, fused = action_of(ref, np.asarray(got["std"], np.float32)[0])
        out["action"] = _ratio(np.abs(a.astype(np.float64) - want), gate) if np.isfinite(a).all() else np.inf
        out["action_is_unfused"] = bool(np.array_equal(a, unfused))
        out["action_is_fused"] = bool(np.array_equal(a, fused))
        if "prev_mean" in got:
            same = np.array_equal(np.asarray(got["prev_mean"], np.float32).view(np.uint32), np.asarray(got["mean"], np.float32).view(np.uint32))
            out["prev_mean"] = 0.0 if same else np.inf
    return out


def worst(ch):
    return max(float(v) for k, v in ch.items() if not k.startswith("action_is"))


# ------------------------------------------------------------------ crafted inputs
VALUE_PATTERNS = ("normal", "all_equal", "tie_block", "zero_mix", "nan_boundary", "inf", "fltmax_inf", "all_negative", "ulp_both_signs",
                  "denormal", "ascending", "descending", "wide_spread")
TIE_PATTERNS = ("all_equal", "tie_block", "zero_mix", "nan_boundary", "fltmax_inf", "denormal")
ACTION_PATTERNS = ("random", "identical", "around_3")


def value_pattern(name, N, K, rng):
    """[N] fp32.  `K` places the tie blocks across the K-th / (K + 1)-th place of the descending order."""
    f = np.float32
    grid = np.linspace(4.0, -4.0, N).astype(f)  # distinct, descending: rank r holds grid[r]
    lo, hi = max(K - 3, 0), min(K + 4, N)       # ranks of the block that straddles the boundary
    perm = rng.permutation(N)
    if name == "normal":
        return (3.0 * rng.standard_normal(N)).astype(f)
    if name == "all_equal":
        return np.full(N, 1.25, f)
    if name == "tie_block":
        v = grid.copy()
        v[lo:hi] = v[lo]
        return v[perm]
    if name == "zero_mix":
        v = np.where(np.arange(N) < lo, np.abs(grid) + 1, -np.abs(grid) - 1).astype(f)
        v[lo:hi] = np.where(rng.random(hi - lo) < 0.5, f(0.0), f(-0.0))
        if hi - lo >= 2:
            v[lo], v[lo + 1] = f(-0.0), f(0.0)
        return v[perm]
    if name == "nan_boundary":
        v = np.where(np.arange(N) < lo, np.abs(grid) + 1, -np.abs(grid) - 1).astype(f)
        v[lo:hi] = np.nan
        return v[perm]
    if name == "inf":
        v = (3.0 * rng.standard_normal(N)).astype(f)
        pos = rng.choice(N, 2, replace=False)  # one of each: no tie (fltmax_inf holds the tied ones)
        v[pos[0]], v[pos[1]] = np.inf, -np.inf
        return v
    if name == "fltmax_inf":
        v = (3.0 * rng.standard_normal(N)).astype(f)
        pos = rng.choice(N, 8, replace=False)
        v[pos[0]], v[pos[1]], v[pos[2]], v[pos[3]] = np.inf, f(FLT_MAX), f(FLT_MAX), np.inf
        v[pos[4]], v[pos[5]], v[pos[6]], v[pos[7]] = -np.inf, f(-FLT_MAX), -np.inf, f(-FLT_MAX)
        return v
    if name == "all_negative":
        return (-10.0 - np.abs(3.0 * rng.standard_normal(N))).astype(f)
    if name == "ulp_both_signs":
        j = np.arange(N)
        mag = (np.float32(1.0).view(np.uint32) + (j // 2).astype(np.uint32)).view(f)  # 1 + (j // 2) ulp
        return np.where(j % 2 == 0, mag, -mag).astype(f)[perm]
    if name == "denormal":
        j = rng.integers(-5, 6, N)
        return (j.astype(np.float64) * 2.0 ** -149).astype(f)
    if name == "ascending":
        return grid[::-1].copy()
    if name == "descending":
        return grid.copy()
    if name == "wide_spread":
        return (1000.0 * rng.standard_normal(N)).astype(f)
    raise KeyError(name)


def action_pattern(name, H, N, A, rng):
    f = np.float32
    if name == "random":
        return rng.uniform(-1.0, 1.0, (H, N, A)).astype(f)
    if name == "identical":  # every sample the same sequence: variance 0, the min_std clamp
        return np.broadcast_to(rng.uniform(-1.0, 1.0, (H, 1, A)).astype(f), (H, N, A)).copy()
    if name == "around_3":  # spreads of +- 3: the max_std clamp
        return (3.0 * np.sign(rng.standard_normal((H, N, A))) + 0.25 * rng.standard_normal((H, N, A))).astype(f)
    raise KeyError(name)


def plans_of(N, K, H, A, seed=0):
    """The plans of one k_refit call at this geometry: every value pattern on random actions, then the two clamping action
    patterns on a continuous and on a tied value pattern.  -> (names, value [E, N], actions [E, H, N, A])."""
    rng = np.random.default_rng([seed, N, K, H, A])
    combos = [(v, "random") for v in VALUE_PATTERNS] + [("normal", "identical"), ("normal", "around_3"), ("tie_block", "identical"),
                                                        ("tie_block", "around_3")]
    vals = np.stack([value_pattern(v, N, K, rng) for v, _ in combos])
    acts = np.stack([action_pattern(a, H, N, A, rng) for _, a in combos])
    return [f"{v}/{a}" for v, a in combos], vals, acts


K_OF = lambda N: (1, 3, 61, 64, N)
GEOMETRY_N = (64, 192, 512, 1024)
GEOMETRY_HA = ((1, 1), (3, 6), (5, 61))
CFG = dict(temperature=0.5, min_std=0.05, max_std=2.0)  # config.yaml:40-42, what named_config gives every handle here


def pick_cases(K, H, N, A, seed=3):
    """The final pick's crafted (value, gumbel_exp, final_eps) rows: name -> dict.  Values are a caller input of shard_refit."""
    rng = np.random.default_rng([seed, K, A])
    f = np.float32
    out = {}
    out["random"] = dict(value=(3.0 * rng.standard_normal(N)).astype(f), gumbel_exp=(rng.exponential(size=K) + 1e-3).astype(f),
                         final_eps=rng.standard_normal(A).astype(f))
    # every score equal (all values equal) and every exponential equal: the first elite, sample row 0
    out["all_tied"] = dict(value=np.full(N, -2.5, f), gumbel_exp=np.full(K, 0.75, f), final_eps=rng.standard_normal(A).astype(f))
    # elites beyond the first three underflow to score 0 (logit -inf) and hold tiny exponentials that would win on any finite logit
    v = np.full(N, -1.0e4, f)
    top = rng.choice(N, min(3, K), replace=False)
    v[top] = np.array([5.0, 4.0, 3.5], f)[:len(top)]
    ex = np.full(K, 1e-30, f)
    ex[:3] = np.array([2.0, 0.05, 1.0], f)[:min(3, K)]
    out["underflow"] = dict(value=v, gumbel_exp=ex, final_eps=rng.standard_normal(A).astype(f))
    # a final noise that drives every action component past +-1
    out["eps_past_one"] = dict(value=(3.0 * rng.standard_normal(N)).astype(f), gumbel_exp=(rng.exponential(size=K) + 1e-3).astype(f),
                               final_eps=(60.0 * np.where(np.arange(A) % 2 == 0, 1.0, -1.0)).astype(f))
    return out
