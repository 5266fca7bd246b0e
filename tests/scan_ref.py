"""float64 restatements of the two operators the engine's launch forms compute (test helper; no tests here).

  selective scan with the dt_proj fused in (csrc/scan.hip), one direction or both, token-major:
      delta = softplus(rnd(dt_low . Wdt^T) + bias);  h_t = exp(delta_t A) (.) h_{t-1} + delta_t B_t u_t;  y_t = <h_t, C_t> + D u_t
  conv1d + SiLU + x_proj of both directions (csrc/convx.hip)

Plain torch on the CPU, every product and sum in float64.  `rnd` is applied where a kernel rounds to its storage dtype (the dt_proj
output, every stored y) and nowhere else, so that what is left between a kernel and this file is the kernel's own fp32 arithmetic.
A walk can start from a given state, cover part of the strand and return its end state and sum of delta: that is what the
segment identity (csrc/scan.hip scan_carry_kernel) and the dropped-carry sensitivity of tests/test_scan_forms.py are built from."""
import math

import torch

N = 16
TB = 32                  # csrc/scan.hip: time steps per delta tile; segments are whole tiles in walk space


def ident(t):
    return t


def bf16(t):
    """round to bf16, keep the dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def split_hi_lo(v):
    """csrc/kernels.hpp, pack.hip section: v (fp32) = hi + lo with hi = bf16(v), lo = bf16(v - hi).  -> (hi, lo) bf16 tensors."""
    v = v.float()
    hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


def hi_rounds_sum(hi, lo):
    """hi == bf16(hi + lo), element-wise (hi + lo is exact in fp32).  One exception is inherent in the definition and allowed:
    when v - hi lies just under half an ulp of hi, lo = bf16(v - hi) rounds UP to exactly half an ulp, hi + lo is then an exact tie
    between two bf16 values and round-to-nearest-even may pick the other one - such elements (the low 16 bits of hi + lo are
    0x8000) pass as long as hi is one of the tie's two neighbours."""
    s = hi.float() + lo.float()
    tie = (s.view(torch.int32) & 0xFFFF) == 0x8000
    near = (s - hi.float()).abs() == lo.float().abs()
    return (s.to(torch.bfloat16) == hi) | (tie & near)


def silu(z):
    z = z.double()
    return z * torch.sigmoid(z)


def softplus(x):
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def delta_of(d, rnd=ident):
    """[S, L, E] float64: softplus(rnd(dt_low . Wdt^T) + bias)"""
    raw = torch.einsum("slr,er->sle", d["dt_low"].double(), d["Wdt"].double())
    return softplus(rnd(raw) + d["dbias"].double())


def walk(d, reverse=False, rnd=ident, steps=None, h0=None, drop_at=()):
    """One direction, ungated.  d: dict(u [S, L, E], dt_low [S, L, R], Wdt [E, R], B, C [S, L, 16], A [E, 16], D, dbias [E]).
    Walk step s visits row t = L - 1 - s (reverse) or s.  steps = (s0, s1): only those walk steps, from state h0 [S, E, 16] (None:
    zero).  drop_at: walk steps before which the state is zeroed (a carry that was lost).
    -> (y [S, L, E] float64, rows outside the walked steps NaN;  end state [S, E, 16];  sum of delta over the walked steps [S, E])"""
    delta = delta_of(d, rnd)
    u, B, C = d["u"].double(), d["B"].double(), d["C"].double()
    A, D = d["A"].double(), d["D"].double()
    S, L, E = u.shape
    s0, s1 = steps if steps is not None else (0, L)
    h = torch.zeros(S, E, N, dtype=torch.float64) if h0 is None else h0.clone()
    y = torch.full((S, L, E), float("nan"), dtype=torch.float64)
    dsum = torch.zeros(S, E, dtype=torch.float64)
    for s in range(s0, min(s1, L)):
        t = L - 1 - s if reverse else s
        if s in drop_at:
            h = torch.zeros_like(h)
        dl = delta[:, t]                                                   # [S, E]
        h = torch.exp(dl[..., None] * A) * h + (dl * u[:, t])[..., None] * B[:, t, None, :]
        y[:, t] = (h * C[:, t, None, :]).sum(-1) + D * u[:, t]
        dsum += dl
    return y, h, dsum


def segment_bounds(L, G, seg_blocks):
    """walk-space [s0, s1) of each of the G segments (csrc/scan.hip: seg_blocks tiles of TB steps each, the last one clipped at L)"""
    return [(g * seg_blocks * TB, min(L, (g + 1) * seg_blocks * TB)) for g in range(G)]


def carried_states(d, bounds, reverse=False, rnd=ident):
    """The identity stated above scan_carry_kernel: every segment walked from a ZERO state gives (h_end, sum delta), and
    h0[g] = exp(A sum_delta[g-1]) (.) h0[g-1] + h_end[g-1], h0[0] = 0.  -> list of h0 per segment."""
    A = d["A"].double()
    h0 = [torch.zeros(d["u"].shape[0], d["u"].shape[2], N, dtype=torch.float64)]
    for (s0, s1) in bounds[:-1]:
        _, hend, dsum = walk(d, reverse, rnd, steps=(s0, s1))
        h0.append(torch.exp(A * dsum[..., None]) * h0[-1] + hend)
    return h0


def walk_cut(d, bounds, reverse=False, rnd=ident):
    """the strand walked segment by segment from the carried states -> y [S, L, E]"""
    h0 = carried_states(d, bounds, reverse, rnd)
    y = None
    for (s0, s1), h in zip(bounds, h0):
        yg, _, _ = walk(d, reverse, rnd, steps=(s0, s1), h0=h)
        y = yg if y is None else torch.where(torch.isnan(y), yg, y)
    return y


def combine(yf, yr, z, mode, rnd=ident, pair=False):
    """Both directions' ungated float64 outputs -> what the launches leave in y, rounded where they round:
      "gate_once"  forward stored ungated, reverse adds its own and gates the sum:  rnd((rnd(yf) + yr) silu(z))
                   pair: on rows >= L / 2 it is the REVERSE direction's first half that was stored: rnd((rnd(yr) + yf) silu(z))
      "gate_each"  rnd(rnd(yf silu(z)) + rnd(yr silu(z)))     (the same two rounded addends in either order)
      "strict"     (rnd(yf silu(z)), rnd(yr silu(z)))"""
    g = silu(z)
    if mode == "strict":
        return rnd(yf * g), rnd(yr * g)
    if mode == "gate_each":
        return rnd(rnd(yf * g) + rnd(yr * g))
    assert mode == "gate_once"
    out = rnd((rnd(yf) + yr) * g)
    if pair:
        h = yf.shape[1] // 2
        out[:, h:] = rnd((rnd(yr) + yf) * g)[:, h:]
    return out


def row_err(got, ref):
    """the per-row metric: max_c |got - ref| / max_c |ref| over the channels of each row (strand, t) -> [S, L] float64"""
    got, ref = got.double().cpu(), ref.double().cpu()
    return (got - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)


# ---- conv1d + SiLU + x_proj, both directions ------------------------------------------------------------------------------------
def conv_silu(x, w, b, reverse=False, rnd=ident):
    """x [S, L, E]; w [E, 4]; b [E] -> rnd(silu(b + sum_k w[k] x[t - 3 + k]))  (reverse: x[t + 3 - k]) [S, L, E] float64"""
    x, w, b = x.double(), w.double(), b.double()
    S, L, E = x.shape
    pad = torch.zeros(S, 3, E, dtype=torch.float64)
    xp = torch.cat([pad, x, pad], dim=1)                                   # row t of x is row t + 3 of xp
    acc = b.expand(S, L, E).clone()
    for k in range(4):
        o = 3 - k if reverse else k - 3
        acc = acc + w[:, k] * xp[:, 3 + o:3 + o + L]
    return rnd(acc * torch.sigmoid(acc))


def conv_xproj(x, wf, bf, wr, br, xpf, xpr, rnd=ident):
    """-> (xc_f, xc_r [S, L, E], x_dbl_f, x_dbl_r [S, L, R + 32]) float64; x_dbl = rnd(xc . x_proj^T) on the ROUNDED xc"""
    xcf, xcr = conv_silu(x, wf, bf, False, rnd), conv_silu(x, wr, br, True, rnd)
    return xcf, xcr, rnd(torch.einsum("sle,re->slr", xcf, xpf.double())), rnd(torch.einsum("sle,re->slr", xcr, xpr.double()))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
N_LATCH = 16             # channels [0, 8): latched by the forward direction, [8, 16): by the reverse direction (see make_direction)
HOT = (16, 17, 18)       # delta + bias > 20: softplus's pass-through branch
COLD = (19, 20, 21)      # delta + bias ~ -12


def make_direction(g, S, L, E, R, bf, reverse=False):
    """One direction's operands (fp32 tensors holding values exact in the model dtype where the engine stores that dtype).
      dt bias: softplus(bias) log-uniform over 1e-3 .. 0.1 (checkpoint.synthetic_state_dict);  A as tests/test_gpu_ops.py _scan_inputs
      HOT: bias 22 (pass-through branch; u scaled down so that these channels do not own every row's maximum);  COLD: bias -12
      latched channels - what makes a lost carry show on every later row, also at bf16's bars: eight channels per direction use the
        scan's selectivity the way a trained model does.  Their bias is -12 (time step 6e-6: the state neither decays nor takes
        input) and their dt_proj row reads one dt_low column that is 4 during the first 32 walk steps and 0 afterwards (weight 3:
        delta + bias = 0, time step ln 2), with u = 7 there: the state is loaded in the first 32 steps and then carried unchanged
        across every segment boundary to the end of the strand (B and C share a sign on states 0 .. 3, so <h, C_t> never averages
        out).  On the rows after the load u is set to -0.6 <h, C_t> / D (D = -4 on these channels), so that the channel's output is
        0.4 of what its carried state contributes: dropping the carry changes the row by about 2.5 times its magnitude.  The other direction's eight channels stay
        shut here (u = 0, time step 6e-6: output 0), so the two directions do not mask each other in the sum."""
    r = (lambda t: t.to(torch.bfloat16).float()) if bf else ident
    u = torch.randn(S, L, E, generator=g)
    dt_low = torch.randn(S, L, R, generator=g)
    Wdt = torch.randn(E, R, generator=g) * R ** -0.5 * 0.5
    B = torch.randn(S, L, N, generator=g)
    C = torch.randn(S, L, N, generator=g)
    A = -torch.exp(torch.log(torch.arange(1, N + 1).float())[None, :] + 0.3 * torch.randn(E, N, generator=g))
    D = torch.rand(E, generator=g) + 0.5
    dt = torch.exp(torch.rand(E, generator=g) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
    dbias = dt + torch.log(-torch.expm1(-dt))
    for c in HOT:
        dbias[c] = 22.0
        u[:, :, c] *= 0.003
    for c in COLD:
        dbias[c] = -12.0
    # latched channels
    own = slice(8, 16) if reverse else slice(0, 8)
    rows = lambda s0, s1: slice(L - s1, L - s0) if reverse else slice(s0, s1)          # memory rows of walk steps [s0, s1)
    load = min(TB, L)
    B[:, :, :4] = 1.5 + 0.1 * B[:, :, :4]
    C[:, :, :4] = 1.5 + 0.1 * C[:, :, :4]
    dbias[:N_LATCH] = -12.0
    D[:N_LATCH] = -4.0                                              # the skip term opposes the state's contribution, also while it is loaded
    Wdt[:N_LATCH] = 0.0
    Wdt[:, 0] = 0.0
    Wdt[own, 0] = 3.0
    dt_low[:, :, 0] = 0.0
    dt_low[:, rows(0, load), 0] = 4.0
    noise = u[:, :, own].clone()
    u[:, :, :N_LATCH] = 0.0
    u[:, rows(0, load), own] = 7.0 + 0.1 * noise[:, rows(0, load)]
    B[:, rows(0, load), 4:] *= 0.1                                  # what is loaded sits in the states whose C has one sign
    C[:, rows(0, load), :4] *= 0.1                                  # ... and shows little while it is being loaded
    d = dict(u=r(u), dt_low=r(dt_low), Wdt=r(Wdt), B=r(B), C=r(C), A=A, D=D, dbias=dbias)
    for _ in range(2 if L > load else 0):      # twice: the little that u itself adds to the state moves <h, C_t>
        later = rows(load, L)
        carried = walk(d, reverse, bf16 if bf else ident)[0][:, later, own] - D[own].double() * d["u"][:, later, own].double()      # <h, C_t>
        u[:, later, own] = (-0.6 * carried / D[own].double()).float()
        d["u"] = r(u)
    return d


def make_case(seed, S, L, E, R, bf=False):
    """-> dict(fwd=direction, rev=direction, z [S, L, E]); the two directions have their own operands, as in the engine.  The gate of
    the latched channels is kept open (z ~ 1.5), so that they show in the gated outputs of every row."""
    g = torch.Generator().manual_seed(seed)
    fwd, rev = make_direction(g, S, L, E, R, bf), make_direction(g, S, L, E, R, bf, reverse=True)
    z = torch.randn(S, L, E, generator=g)
    z[:, :, :N_LATCH] = 1.5 + 0.1 * z[:, :, :N_LATCH]
    return dict(fwd=fwd, rev=rev, z=z.to(torch.bfloat16).float() if bf else z)


# ---- the cases of tests/test_gpu_engine_forms.py, and the bars they are held to ----------------------------------------------------
# (tests/test_scan_forms.py checks on the CPU that each shape gives the stated form and that the inputs are sensitive to a lost carry)
# segmented: (S, L, E) -> (G segments, 32-step blocks per segment)
SEG_SHAPES = {(2, 256, 128): (8, 1), (2, 296, 128): (10, 1), (2, 300, 128): (10, 1), (2, 544, 128): (9, 2), (1, 2072, 64): (4, 17)}
PAIR_SHAPES = [(S, L, 128) for L in (128, 192, 256) for S in (1, 3)]
PLAIN_L = (8, 40, 44, 64, 256)                               # S = 2, E = 128; 44: not a multiple of 8
CONVX_KS = {(256, True): 2, (256, False): 4, (384, True): 3, (384, False): 6}      # (E, bf16) -> K-split factor at S = 2, L in CONVX_L
CONVX_L = (1, 127, 129)
R_OF = {64: 24, 96: 80}                                      # the dt_rank used for each padded dt_rank Rp
# the project's own bars (tests/test_gpu_ops.py): test_selective_scan_fused_dtproj, test_conv_xproj_fused, test_linear_split
BAR_SCAN = {False: 3e-5, True: 2.0 ** -7}                    # [bf16]; sums of two rounded directions: twice that
BAR_CONV = {False: 1e-5, True: 2.0 ** -7}
BAR_XDBL = {False: 3e-5, True: 2.0 ** -7}
BAR_SPLIT = 2e-5
ORACLE_FACTOR = 8                                            # fp32: max(project bar, 8 x the fp32 CPU oracle's own worst row)

_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def case_for(S, L, E, Rp, bf):
    return cached(("case", S, L, E, Rp, bf), lambda: make_case(1000 * S + L + Rp, S, L, E, R_OF[Rp], bf))


def walks_for(S, L, E, Rp, bf):
    """(case, yf, yr): both directions' ungated float64 outputs, the dt_proj output rounded as the model dtype rounds it"""
    def run():
        case = case_for(S, L, E, Rp, bf)
        rnd = bf16 if bf else ident
        return case, walk(case["fwd"], False, rnd)[0], walk(case["rev"], True, rnd)[0]
    return cached(("walks", S, L, E, Rp, bf), run)


def oracle_walks(S, L, E, Rp):
    """the fp32 CPU oracle (oracle/caduceus_oracle.py selective_scan_fn) on the fp32 case: both directions' ungated outputs [S, L, E]"""
    def run():
        from oracle import caduceus_oracle as O
        case = case_for(S, L, E, Rp, False)
        out = []
        for d, rev in ((case["fwd"], False), (case["rev"], True)):
            f = (lambda t: t.flip(1)) if rev else ident
            delta = torch.einsum("slr,er->sle", d["dt_low"], d["Wdt"])
            y = O.selective_scan_fn(f(d["u"]).transpose(1, 2), f(delta).transpose(1, 2), d["A"], f(d["B"]).transpose(1, 2),
                                    f(d["C"]).transpose(1, 2), d["D"], z=None, delta_bias=d["dbias"], delta_softplus=True)
            out.append(f(y.transpose(1, 2)))
        return out
    return cached(("oracle", S, L, E, Rp), run)


def scan_bar(S, L, E, Rp, bf, mode):
    """the bar of one scan case.  mode: "fwd" / "rev" (one direction, ungated), "strict" (one direction gated), "gate_once", "gate_each"
    (sums: twice the single-direction bar).  fp32: max(project bar, 8 x the fp32 oracle's worst row against float64), the oracle's
    outputs combined in fp32 as the launch combines them."""
    base = BAR_SCAN[bf] * (2 if mode in ("gate_once", "gate_each") else 1)
    if bf:
        return base

    def run():
        case, yf, yr = walks_for(S, L, E, Rp, False)
        of, orv = oracle_walks(S, L, E, Rp)
        g = case["z"] * torch.sigmoid(case["z"])
        if mode == "fwd":
            dev = row_err(of, yf)
        elif mode == "rev":
            dev = row_err(orv, yr)
        elif mode == "strict":
            dev = torch.maximum(row_err(of * g, yf * silu(case["z"])), row_err(orv * g, yr * silu(case["z"])))
        elif mode == "gate_once":
            dev = row_err((of + orv) * g, combine(yf, yr, case["z"], "gate_once"))
        else:
            dev = row_err(of * g + orv * g, combine(yf, yr, case["z"], "gate_each"))
        return max(base, ORACLE_FACTOR * dev.max().item())
    return cached(("bar", S, L, E, Rp, mode), run)
