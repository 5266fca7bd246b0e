"""Operator-level mirrors of the third-party functions the reference's hot path calls, running on the
MI355X HIP kernels through the C ABI.  Same names, argument meaning and layouts as the originals
 so the parity tests read like the upstream operators' own tests:

  rms_norm_fn(x, weight, bias, residual, eps, prenorm, residual_in_fp32)   mamba_ssm.ops.triton.layer_norm
  causal_conv1d_fn(x, weight, bias, activation)                            causal_conv1d 1.4.0
  selective_scan_fn(u, delta, A, B, C, D, z, delta_bias, delta_softplus)   mamba_ssm 2.2.2
  mamba_inner_fn(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A, ...)
                                                                           mamba_ssm 2.2.2 (the call Mamba.forward's fast path makes)
  linear(x, weight)                                                        F.linear (no bias)

Inputs use the reference's channels-first (B, E, L) layout where the originals do; they are transposed
to the engine's token-major layout here (test plumbing — the engine itself never transposes).
All tensors must be ROCm tensors; there is no CPU fallback.

Differentiable (each a torch.autograd.Function on this project's backward kernels as soon as grad mode is on and an input requires
grad; otherwise the plain call, no graph): selective_scan_fn (include/pcad_train.h), causal_conv1d_fn / causal_conv1d_dir and
rms_norm_fn (include/pcad_bwd.h), mamba_inner_fn as a composition of those around stock F.linear, mlm_loss_head_fn - the end of the
masked LM's forward with labels (include/pcad_bwd.h pcad_loss_head_bwd) - and pooled_head_fn, the end of the sequence classifier's
(include/pcad_bwd.h pcad_pooled_head_bwd) - with pooled_logits_fn, that head's score part alone on cached pooled vectors
(pcad_pooled_logits(_bwd); §4x); lora_linear_fn is a frozen linear with LoRA factors merged in, differentiated by torch matmuls;
lora_dropout_linear_fn is the unmerged form with a dropout on the branch's input, on the masked rank-r kernels (pcad_lora_down(_bwd); §4u).
plantcaduceus_amd.training composes the models from them.  linear_fn is F.linear for the masked LM's projections; for a weight that
carries an fp32 `main_grad` its backward adds dy^T x to that buffer with linear_wgrad (include/pcad_bwd.h pcad_linear_wgrad).
"""
from __future__ import annotations

import ctypes as C
import logging
from types import SimpleNamespace
from typing import Optional

import torch

import torch.nn.functional as F

from .engine import (MAX_LABELS, POOLING, _DT, _check, _require_gpu, _stream_ptr, load_bwd_library, load_library,
                     load_train_library)


def _dt(t: torch.Tensor) -> int:
    if t.dtype not in _DT:
        raise ValueError(f"unsupported dtype {t.dtype}")
    return _DT[t.dtype]


def _ptr(t: Optional[torch.Tensor]):
    """an optional operand as the C ABI takes it: its address, or NULL"""
    return t.data_ptr() if t is not None else None


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _scratch(nb: int, dev, poison: bool = False):
    """a scratch of nb bytes -> (the uint8 tensor that keeps the memory alive, the 256-byte aligned address of nb bytes inside it).
    poison (tests): every byte starts as 0xFF - NaN in fp32 and bf16 -, so that a slot read without having been written shows."""
    if poison:
        buf = torch.full((nb + 256,), 0xFF, dtype=torch.uint8, device=dev)
    else:
        buf = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
    return buf, _round_up(buf.data_ptr(), 256)


# ---- guarded outputs (the poison forms, tests): an output is NaN where the kernel must write it and lies inside a larger buffer of
# ---- sentinels, so that a row the kernel skipped and a store outside the output both show -------------------------------------------
GUARD = -1024.0          # the sentinel: exact in bf16 and fp32
OPTIM_GUARD = 64         # sentinel elements around every output of the optimizer's poison forms (a multiple of 16 bytes in either dtype)


def _guard_elems(shape, geometry: str) -> int:
    """sentinel elements before and after an output of `shape`.  "row": one row of the output, as many elements as its last dimension;
    "lines": the row rounded up to whole 128-byte lines of bf16, so that a GEMM output keeps its alignment; "optim": OPTIM_GUARD."""
    return {"row": shape[-1], "lines": _round_up(shape[-1], 64), "optim": OPTIM_GUARD}[geometry]


def _guarded(shape, dtype, dev, geometry: str = "row", poison: bool = True):
    """an output buffer -> (tensor of `shape`, the whole buffer or None).  poison: NaN inside, `_guard_elems` sentinels before and after;
    else plain torch.empty and no buffer around it."""
    if not poison:
        return torch.empty(shape, dtype=dtype, device=dev), None
    n, g = 1, _guard_elems(shape, geometry)
    for k in shape:
        n *= k
    whole = torch.full((n + 2 * g,), GUARD, dtype=dtype, device=dev)
    whole[g:g + n] = float("nan")
    return whole[g:g + n].view(shape), whole


def _guarded_copy(t: torch.Tensor, geometry: str = "optim"):
    """-> (a copy of t between sentinels, the whole buffer)"""
    c, whole = _guarded(t.shape, t.dtype, t.device, geometry)
    c.copy_(t.detach())
    return c, whole


def _guards_intact(outs) -> bool:
    """outs: (tensor, whole buffer or None) pairs: whether every element of a whole buffer outside its tensor still is the sentinel
    (the tensor any view of the buffer: `_guarded`'s, or linear_wgrad's 2-D frame).  Reads the device; free without buffers."""
    ok = True
    for t, whole in outs:
        if whole is not None:
            outside = torch.ones_like(whole, dtype=torch.bool)
            outside.as_strided(t.shape, t.stride(), t.storage_offset()).fill_(False)
            ok = ok and bool((whole[outside] == GUARD).all())
    return ok


def _guarded_copies(tensors, back, blank: bool = False):
    """the poison forms of the in-place operators run on copies: -> one copy between OPTIM_GUARD sentinels per tensor (None stays None;
    blank: NaN instead of the tensor's values); `back` collects the (tensor, copy, whole buffer) triples `_copy_back` takes"""
    copies = []
    for t in tensors:
        c = None
        if t is not None:
            c, whole = _guarded(t.shape, t.dtype, t.device, "optim") if blank else _guarded_copy(t)
            back.append((t, c, whole))
        copies.append(c)
    return copies


def _copy_back(back) -> bool:
    """the results of a poisoned run from the copies into the tensors they stand for -> whether all sentinels are intact"""
    with torch.no_grad():
        for t, c, _ in back:
            t.copy_(c)
    return _guards_intact([(c, whole) for _, c, whole in back])


def _residual_dtype(x_dtype, residual_in_fp32):
    """the dtype of the residual stream: fp32 with residual_in_fp32 or an fp32 x, else x's"""
    return torch.float32 if (residual_in_fp32 or x_dtype == torch.float32) else x_dtype


def rms_norm_fn(x, weight, bias=None, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False):
    """When x, weight or residual requires grad the call is differentiable (pcad_add_rmsnorm_bwd): each gradient comes back in its
    input's shape and dtype; the prenorm output carries its own gradient into the residual stream."""
    _require_gpu(x, "x")
    if bias is not None:
        raise NotImplementedError("RMSNorm bias is not used by Caduceus")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, residual)):
        # the casts stay torch ops outside the Function, so that autograd returns each gradient in its input's dtype
        rdt = _residual_dtype(x.dtype, residual_in_fp32)
        y, res_out = _RmsNormFn.apply(x, weight.float(), residual.to(rdt) if residual is not None else None, float(eps),
                                      bool(residual_in_fp32))
        return (y, res_out) if prenorm else y
    return _rms_norm_forward(x, weight, residual, eps, prenorm, residual_in_fp32)


def _rms_norm_forward(x, weight, residual, eps, prenorm, residual_in_fp32):
    lib = load_library()
    D = x.shape[-1]
    xf = x.contiguous().view(-1, D)
    rows = xf.shape[0]
    rdt = _residual_dtype(x.dtype, residual_in_fp32)
    res_in = residual.to(rdt).contiguous().view(-1, D) if residual is not None else None
    y = torch.empty_like(xf)
    res_out = torch.empty((rows, D), dtype=rdt, device=x.device)
    w = weight.float().contiguous()
    with torch.cuda.device(x.device):
        _check(lib.pcad_add_rmsnorm(xf.data_ptr(), _ptr(res_in), w.data_ptr(), y.data_ptr(), res_out.data_ptr(), rows, D, float(eps),
                                    _dt(xf), _DT[rdt], _stream_ptr()), "pcad_add_rmsnorm")
    y = y.view(x.shape)
    return (y, res_out.view(x.shape)) if prenorm else y


def _conv_taps(E, w_fwd, b_fwd, w_rev, b_rev):
    """the conv parameters of both directions as the kernels take them: fp32 (w_fwd [E, 4], b_fwd [E], w_rev [E, 4], b_rev [E])"""
    return [t.float().contiguous() for t in (w_fwd.reshape(E, -1), b_fwd, w_rev.reshape(E, -1), b_rev)]


def causal_conv1d_bidir(x_tm, w_fwd, b_fwd, w_rev, b_rev):
    """Token-major both-direction form used by the engine: x_tm [S, L, E] -> (y_fwd, y_rev) [S, L, E]."""
    _require_gpu(x_tm, "x")
    lib = load_library()
    S, L, E = x_tm.shape
    x_tm = x_tm.contiguous()
    yf = torch.empty_like(x_tm)
    yr = torch.empty_like(x_tm)
    taps = _conv_taps(E, w_fwd, b_fwd, w_rev, b_rev)
    with torch.cuda.device(x_tm.device):
        _check(lib.pcad_causal_conv1d_silu(x_tm.data_ptr(), E, *[t.data_ptr() for t in taps], yf.data_ptr(), yr.data_ptr(),
                                           S, L, E, _dt(x_tm), _stream_ptr()), "pcad_causal_conv1d_silu")
    return yf, yr


def to_blocked(x_rows: torch.Tensor, pad_value: float = 0.0) -> torch.Tensor:
    """[rows, E] -> the engine's blocked layout [rows8/8, E*esz/128, 8, 128/esz] (include/pcad.h), rows padded to 8 with pad_value."""
    rows, E = x_rows.shape
    per = 128 // x_rows.element_size()
    if E % per:
        raise ValueError("E * elem must be a multiple of 128 bytes")
    rows8 = _round_up(rows, 8)
    buf = torch.full((rows8, E), pad_value, dtype=x_rows.dtype, device=x_rows.device)
    buf[:rows] = x_rows
    return buf.view(rows8 // 8, 8, E // per, per).permute(0, 2, 1, 3).contiguous()


def from_blocked(xb: torch.Tensor, rows: int) -> torch.Tensor:
    nb, pieces, _, per = xb.shape
    return xb.permute(0, 2, 1, 3).reshape(nb * 8, pieces * per)[:rows].contiguous()


def _split_blocked(xb: torch.Tensor, rows: int):
    """a blocked buffer -> (its `rows` rows as plain rows, its padding rows)"""
    full = from_blocked(xb, xb.shape[0] * 8)
    return full[:rows].contiguous(), full[rows:].contiguous()


def causal_conv1d_dir(x_tm, weight, bias, reverse: bool = False, blocked: bool = False):
    """One direction of the conv (pcad_causal_conv1d_silu_dir, what "untied_directions" runs per direction): x_tm [S, L, E] ->
    y [S, L, E]; reverse: anti-causal (the causal conv of the flipped strand, flipped back).  blocked: x is handed over and y is
    returned through the engine's blocked layout (`to_blocked` / `from_blocked`) instead of plain rows.
    When x_tm, weight or bias requires grad the call is differentiable (pcad_causal_conv1d_silu_bwd), plain layout only."""
    _require_gpu(x_tm, "x")
    S, L, E = x_tm.shape
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x_tm, weight, bias)):
        if blocked:
            raise NotImplementedError("the blocked layout is an inference form: with an input that requires grad, use plain rows")
        return _CausalConv1dDirFn.apply(x_tm, weight.reshape(E, -1).float(), bias.float(), bool(reverse))
    return _causal_conv1d_dir_forward(x_tm, weight, bias, reverse, blocked)


def _causal_conv1d_dir_forward(x_tm, weight, bias, reverse, blocked):
    lib = load_library()
    S, L, E = x_tm.shape
    w = weight.reshape(E, -1).float().contiguous()
    b = bias.float().contiguous()
    with torch.cuda.device(x_tm.device):
        xin = to_blocked(x_tm.reshape(S * L, E)) if blocked else x_tm.contiguous()
        # NaN where the kernel must write, so that a row it skipped shows; a blocked buffer's padding rows are not its to write
        yb = torch.full_like(xin, float("nan"))
        _check(lib.pcad_causal_conv1d_silu_dir(xin.data_ptr(), E, w.data_ptr(), b.data_ptr(), yb.data_ptr(), E, S, L, E, int(bool(reverse)),
                                               int(blocked), int(blocked), _dt(x_tm), _stream_ptr()), "pcad_causal_conv1d_silu_dir")
    return from_blocked(yb, S * L).view(S, L, E) if blocked else yb


def padded_dt_rank(R: int) -> int:
    """csrc/kernels.hpp padded_dt_rank: the columns dt_low and W_dt are zero padded to - 64, beyond that a multiple of 32"""
    return 64 if R <= 64 else _round_up(R, 32)


def pack_x_proj(w, R: int, Rp: int, E: int, dtype, dev):
    """x_proj's weight [R + 32, E] as the fused kernel takes it, [Rp + 32, E] in `dtype`: the dt rows, zero rows up to Rp, the B | C rows"""
    p = torch.zeros((Rp + 32, E), dtype=dtype, device=dev)
    p[:R] = w[:R].to(dtype)
    p[Rp:] = w[R:].to(dtype)
    return p


def _conv_xproj_operands(x_tm, w_fwd, b_fwd, w_rev, b_rev, x_proj_fwd, x_proj_rev):
    """what both forms of the fused conv + x_proj take: -> (x blocked, the conv taps, the packed x_proj weights (fwd, rev), R, Rp)"""
    S, L, E = x_tm.shape
    R = x_proj_fwd.shape[0] - 32
    if not 0 < R <= 96:
        raise ValueError("dt_rank must be in [1, 96] for the fused kernel")
    Rp = padded_dt_rank(R)
    xb = to_blocked(x_tm.reshape(S * L, E))
    wx = [pack_x_proj(w, R, Rp, E, x_tm.dtype, x_tm.device) for w in (x_proj_fwd, x_proj_rev)]
    return xb, _conv_taps(E, w_fwd, b_fwd, w_rev, b_rev), wx, R, Rp


def _conv_xproj_raw(x_tm, w_fwd, b_fwd, w_rev, b_rev, x_proj_fwd, x_proj_rev):
    """pcad_conv_xproj_bidir on a token-major x [S, L, E]: -> (xc [2] blocked, dtl [2] [rows, Rp], bc [2] fp32 [rows, 32], R, Rp)."""
    _require_gpu(x_tm, "x")
    lib = load_library()
    S, L, E = x_tm.shape
    dt, dev, rows = x_tm.dtype, x_tm.device, S * L
    xb, taps, wx, R, Rp = _conv_xproj_operands(x_tm, w_fwd, b_fwd, w_rev, b_rev, x_proj_fwd, x_proj_rev)
    scratch, scratch_ptr = _scratch(lib.pcad_conv_xproj_scratch_bytes(E, _DT[dt]), dev)
    xc = [torch.zeros_like(xb) for _ in range(2)]
    dtl = [torch.empty((rows, Rp), dtype=dt, device=dev) for _ in range(2)]
    bc = [torch.empty((rows, 32), dtype=torch.float32, device=dev) for _ in range(2)]
    with torch.cuda.device(dev):
        _check(lib.pcad_conv_xproj_bidir(xb.data_ptr(), *[t.data_ptr() for t in taps], wx[0].data_ptr(), wx[1].data_ptr(), scratch_ptr,
                                         xc[0].data_ptr(), dtl[0].data_ptr(), bc[0].data_ptr(),
                                         xc[1].data_ptr(), dtl[1].data_ptr(), bc[1].data_ptr(),
                                         S, L, E, Rp, _DT[dt], _stream_ptr()), "pcad_conv_xproj_bidir")
    return xc, dtl, bc, R, Rp


def conv_xproj_bidir(x_tm, w_fwd, b_fwd, w_rev, b_rev, x_proj_fwd, x_proj_rev):
    """The engine's fused head of mamba_inner_fn, both directions from one read of x:
        xc_d    = causal_conv1d_fn(x, w_d, b_d, "silu")        (d = rev: anti-causal on the same rows)
        x_dbl_d = F.linear(xc_d, x_proj_d)                     (stored in the model dtype)
    x_tm [S, L, E]; w_* [E, 4]; b_* [E]; x_proj_* [R + 32, E] with R <= 96.
    Returns (xc_fwd, xc_rev [S, L, E], x_dbl_fwd, x_dbl_rev [S, L, R + 32]) in x's dtype."""
    S, L, E = x_tm.shape
    dt = x_tm.dtype
    rows = S * L
    xc, dtl, bc, R, Rp = _conv_xproj_raw(x_tm, w_fwd, b_fwd, w_rev, b_rev, x_proj_fwd, x_proj_rev)
    outs = [from_blocked(c, rows).view(S, L, E) for c in xc]
    dbl = [torch.cat([dtl[d][:, :R], bc[d].to(dt)], dim=1).view(S, L, R + 32) for d in range(2)]
    return outs[0], outs[1], dbl[0], dbl[1]


# ---- the engine's launch forms as operators (include/pcad.h pcad_*_engine / pcad_selective_scan_pair) ----------------------------
# Token-major tensors in and out; the blocked layouts are made and undone here.  Every output buffer starts as NaN where the kernel
# must write it, so that a row it skipped - or a scratch slot it read without writing - shows.
def _y_blocked(y_prior, S, L, E, dt, dev):
    """the blocked y buffer: the caller's prior content (accumulate modes, walk_len), else NaN; padding rows always NaN"""
    if y_prior is None:
        y_prior = torch.full((S, L, E), float("nan"), dtype=dt, device=dev)
    return to_blocked(y_prior.to(dt).reshape(S * L, E), pad_value=float("nan"))


def _ysplit_buffer(rows, E, dev):
    """the ysplit output, NaN: bf16 [rows8, 2E] blocked = [hi | lo]"""
    return torch.full((_round_up(rows, 8) // 8, 2 * E * 2 // 128, 8, 64), float("nan"), dtype=torch.bfloat16, device=dev)


def _decode_y(yb, ysb, S, L, E):
    """the scan forms' blocked outputs -> dict(y [S, L, E], pad: the blocked y buffer's padding rows, hi / lo [S, L, E] bf16: the halves
    of the ysplit buffer, None without one)"""
    y, pad = _split_blocked(yb, S * L)
    hi = lo = None
    if ysb is not None:
        flat = from_blocked(ysb, S * L)
        hi, lo = flat[:, :E].reshape(S, L, E), flat[:, E:].reshape(S, L, E)
    return dict(y=y.view(S, L, E), pad=pad, hi=hi, lo=lo)


def selective_scan_engine(u, dt_low, Wdt, Rp, bc, A2, D, delta_bias, z=None, y_prior=None, reverse=False, accumulate=0, a_scale=1.0,
                          segmented=False, policy_S=0, walk_len=0, ysplit=False, dt_split=False):
    """pcad_selective_scan_engine: one direction's fused dt_proj + scan in the engine's layouts.
    u, z, y_prior [S, L, E] (z / y_prior may be None); dt_low [S, L, lddt] and Wdt [E, Rp] in u's dtype, zero padded to Rp - or, dt_split,
    the bf16 [hi | lo] forms [S, L, 2 Rp] / [E, 2 Rp]; bc fp32 [S, L, 32]; A2 fp32 [E, 16] with the decay rate A2 * a_scale in base 2.
    segmented: hand over the segment scratch (whether the walk is then cut is the library's policy for the shape, see
    pcad_scan_segment_scratch_bytes).  -> namespace(y [S, L, E], pad: the blocked y buffer's padding rows, hi / lo [S, L, E] bf16 or
    None: the ysplit output, seg_bytes)."""
    _require_gpu(u, "u")
    lib = load_library()
    S, L, E = u.shape
    dt, dev, rows = u.dtype, u.device, S * L
    ub = to_blocked(u.reshape(rows, E))
    zb = to_blocked(z.to(dt).reshape(rows, E)) if z is not None else None
    yb = _y_blocked(y_prior, S, L, E, dt, dev)
    dl, W = dt_low.contiguous(), Wdt.contiguous()
    f32 = [t.float().contiguous() for t in (bc, A2, D, delta_bias)]
    seg_bytes = lib.pcad_scan_segment_scratch_bytes(S, L, E, policy_S)
    seg, seg_ptr = _scratch(seg_bytes, dev, poison=True) if segmented else (None, None)
    ysb = _ysplit_buffer(rows, E, dev) if ysplit else None
    with torch.cuda.device(dev):
        _check(lib.pcad_selective_scan_engine(ub.data_ptr(), dl.data_ptr(), dl.shape[-1], W.data_ptr(), Rp, _ptr(zb),
                                              f32[0].data_ptr(), f32[1].data_ptr(), float(a_scale), f32[2].data_ptr(), f32[3].data_ptr(),
                                              yb.data_ptr(), _ptr(ysb), seg_ptr, seg_bytes, policy_S, walk_len, int(bool(dt_split)),
                                              S, L, E, int(bool(reverse)), accumulate, _dt(u), _stream_ptr()), "pcad_selective_scan_engine")
    return SimpleNamespace(**_decode_y(yb, ysb, S, L, E), seg_bytes=seg_bytes)


def selective_scan_pair(fwd, rev, z, Rp, gate_each=False, phases=(3,), ysplit=False, dt_split=False):
    """pcad_selective_scan_pair: both directions in one launch, half a strand each.  fwd / rev: dicts of one direction's operands
    (u [S, L, E], dt_low, Wdt, bc, A2 - scaled by log2(e) -, D, delta_bias, as selective_scan_engine takes them); z [S, L, E].
    phases: the calls to issue in order, (1, 2) as the engine does or (3,).  -> namespace(y [S, L, E], pad, hi, lo)."""
    _require_gpu(z, "z")
    lib = load_library()
    S, L, E = z.shape
    dt, dev, rows = z.dtype, z.device, S * L
    ops = []
    for d in (fwd, rev):
        ops += [to_blocked(d["u"].to(dt).reshape(rows, E)), d["dt_low"].contiguous(), d["Wdt"].contiguous()]
        ops += [d[k].float().contiguous() for k in ("bc", "A2", "D", "delta_bias")]
    zb = to_blocked(z.reshape(rows, E))
    yb = _y_blocked(None, S, L, E, dt, dev)
    ws_bytes = lib.pcad_scan_pair_scratch_bytes(S, E)
    ws, ws_ptr = _scratch(ws_bytes, dev, poison=True)
    ysb = _ysplit_buffer(rows, E, dev) if ysplit else None
    with torch.cuda.device(dev):
        for ph in phases:
            _check(lib.pcad_selective_scan_pair(*[t.data_ptr() for t in ops], zb.data_ptr(), fwd["dt_low"].shape[-1], Rp, yb.data_ptr(),
                                                _ptr(ysb), ws_ptr, ws_bytes, S, L, E, int(bool(gate_each)), int(ph), int(bool(dt_split)),
                                                _DT[dt], _stream_ptr()), "pcad_selective_scan_pair")
    return SimpleNamespace(**_decode_y(yb, ysb, S, L, E))


def conv_xproj_bidir_engine(x_tm, w_fwd, b_fwd, w_rev, b_rev, x_proj_fwd, x_proj_rev, ksplit=True, policy_S=0, split=False):
    """pcad_conv_xproj_bidir_engine on a token-major x [S, L, E] (operands as conv_xproj_bidir's).  ksplit: hand over the K-split
    scratch (whether the launch is then split is the library's policy for the shape); split (fp32): dtl_split + w_split.
    -> namespace(xc (fwd, rev) [S, L, E]; dtl (fwd, rev): [S*L, Rp] in x's dtype, or - split - bf16 [S*L, 2 Rp] = [hi | lo];
                 bc (fwd, rev) fp32 [S*L, 32]; R, Rp; part_bytes: the K-split scratch of this shape, 0 = not split)."""
    _require_gpu(x_tm, "x")
    lib = load_library()
    S, L, E = x_tm.shape
    dt, dev, rows = x_tm.dtype, x_tm.device, S * L
    xb, taps, wx, R, Rp = _conv_xproj_operands(x_tm, w_fwd, b_fwd, w_rev, b_rev, x_proj_fwd, x_proj_rev)
    sb = _round_up(lib.pcad_conv_xproj_scratch_bytes(E, _DT[dt]), 256) + (2 * (Rp + 32) * 2 * E * 2 if split else 0)
    scratch, scratch_ptr = _scratch(sb, dev)
    part_bytes = lib.pcad_conv_xproj_split_scratch_bytes(S, L, E, _DT[dt], Rp, policy_S)
    part, part_ptr = _scratch(part_bytes, dev, poison=True) if ksplit else (None, None)
    xc = [torch.full_like(xb, float("nan")) for _ in range(2)]
    if split:
        dtl = [torch.full((rows, 2 * Rp), float("nan"), dtype=torch.bfloat16, device=dev) for _ in range(2)]
    else:
        dtl = [torch.full((rows, Rp), float("nan"), dtype=dt, device=dev) for _ in range(2)]
    bc = [torch.full((rows, 32), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    with torch.cuda.device(dev):
        _check(lib.pcad_conv_xproj_bidir_engine(xb.data_ptr(), *[t.data_ptr() for t in taps], wx[0].data_ptr(), wx[1].data_ptr(), scratch_ptr, sb,
                                                xc[0].data_ptr(), dtl[0].data_ptr(), bc[0].data_ptr(), xc[1].data_ptr(), dtl[1].data_ptr(),
                                                bc[1].data_ptr(), part_ptr, part_bytes, policy_S,
                                                int(bool(split)), int(bool(split)), S, L, E, Rp, _DT[dt], _stream_ptr()),
               "pcad_conv_xproj_bidir_engine")
    return SimpleNamespace(xc=tuple(from_blocked(c, rows).view(S, L, E) for c in xc), dtl=tuple(dtl), bc=tuple(bc), R=R, Rp=Rp,
                           part_bytes=part_bytes)


def causal_conv1d_fn(x, weight, bias=None, activation=None):
    """x (B, E, L), weight (E, W=4), bias (E), activation must be "silu".  When x, weight or bias requires grad the call is
    differentiable: the one-direction kernel, whose values are the both-direction kernel's bit for bit (csrc/conv.hip), with
    pcad_causal_conv1d_silu_bwd behind it."""
    if activation not in ("silu", "swish"):
        raise NotImplementedError("only activation='silu' is on the Caduceus path")
    if weight.shape[-1] != 4:
        raise NotImplementedError("only conv width 4")
    if bias is None:
        bias = torch.zeros(weight.shape[0], device=x.device)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, weight, bias)):
        return causal_conv1d_dir(x.transpose(1, 2), weight, bias, False).transpose(1, 2)
    yf, _ = causal_conv1d_bidir(x.transpose(1, 2), weight, bias, weight, bias)
    return yf.transpose(1, 2)


def _scan_common(u, B, C, A, D, z, delta_bias):
    Bsz, E, L = u.shape
    dt = u.dtype
    u_tm = u.transpose(1, 2).contiguous()
    z_tm = z.to(dt).transpose(1, 2).contiguous() if z is not None else None
    # B_t | C_t rows in fp32 holding the values at the model dtype's precision (what the x_proj epilogue writes)
    bc = torch.cat([B.to(dt).transpose(1, 2), C.to(dt).transpose(1, 2)], dim=-1).float().contiguous()   # [B, L, 32]
    return (u_tm, z_tm, bc) + _scan_params(A, D, delta_bias, E, u.device)


def _scan_params(A, D, delta_bias, E, dev):
    """A, D and delta_bias as the scan kernels take them: fp32, a missing D or delta_bias as zeros"""
    A32 = A.float().contiguous()
    Dv = (D.float() if D is not None else torch.zeros(E, device=dev)).contiguous()
    db = (delta_bias.float() if delta_bias is not None else torch.zeros(E, device=dev)).contiguous()
    return A32, Dv, db


def _acc_mode(accumulate_into, gate_sum) -> int:
    if accumulate_into is None:
        if gate_sum:
            raise ValueError("gate_sum needs accumulate_into (the other direction's ungated output)")
        return 0
    return 2 if gate_sum else 1


SCAN_BWD_CHUNK = 8       # csrc/kernels.hpp SCAN_BWD_CHUNK: walk steps between two states the backward stores (and re-runs at once)
SCAN_BWD_MAX_SEGMENTS = 64      # csrc/kernels.hpp SCAN_BWD_MAX_SEGMENTS
# the shortest segment the "auto" policy cuts a strand into: a multiple of SCAN_BWD_CHUNK, the shortest length at which doubling the
# segments was not slower for shapes below the slot count (profiles/scan_bwd_seg_timing.txt)
SCAN_BWD_SEG_MIN_STEPS = 128


def scan_bwd_seg_steps(L: int, segments: int) -> int:
    """include/pcad_bwd.h pcad_selective_scan_bwd_seg_steps restated on the host: walk steps per segment, 0 = refused"""
    if L < 1 or not 1 <= segments <= SCAN_BWD_MAX_SEGMENTS:
        return 0
    T = SCAN_BWD_CHUNK
    return T * (-(-(-(-L // segments)) // T))


def scan_bwd_auto_segments(S: int, L: int, E: int, wave_slots: Optional[int] = None) -> int:
    """The `segments="auto"` policy of selective_scan_bwd, a pure function of the shape: the smallest power of two G <= 64 with
    S * (E / 64) * G >= wave_slots (one wave walks 64 channels of one segment), halved while a segment would be shorter than
    SCAN_BWD_SEG_MIN_STEPS.  wave_slots: the waves the device keeps busy at once, by default 8 x its compute units."""
    if wave_slots is None:
        wave_slots = 8 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    waves = max(1, S * (E // 64))
    G = 1
    while G < SCAN_BWD_MAX_SEGMENTS and waves * G < wave_slots:
        G *= 2
    while G > 1 and scan_bwd_seg_steps(L, G) < SCAN_BWD_SEG_MIN_STEPS:
        G //= 2
    return G


# the fewest segments that must be needed to fill the wave slots before the "auto" policy cuts the FORWARD at all: the segmented forward
# walks every step twice (local pass, then walk) at 1.8x the plain kernel's time per step, so 2 segments are slower than none at every
# shape and 4 about even; shapes whose strands fill the slots with 4 or fewer lost or gained nothing (profiles/scan_fwd_seg_timing.txt,
# S = 32)
SCAN_FWD_SEG_MIN_FILL = 8


def scan_fwd_auto_segments(S: int, L: int, E: int, wave_slots: Optional[int] = None) -> int:
    """The `fwd_segments="auto"` policy, a pure function of the shape: scan_bwd_auto_segments' value, except 1 where fewer than
    SCAN_FWD_SEG_MIN_FILL segments already fill the wave slots (S * (E / 64) * SCAN_FWD_SEG_MIN_FILL / 2 >= wave_slots)."""
    if wave_slots is None:
        wave_slots = 8 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    if max(1, S * (E // 64)) * (SCAN_FWD_SEG_MIN_FILL // 2) >= wave_slots:
        return 1
    return scan_bwd_auto_segments(S, L, E, wave_slots)


def _check_segments(segments):
    """`segments` as a caller gives it -> "auto" or an int in [1, 64]; anything else raises ValueError"""
    if isinstance(segments, str):
        if segments == "auto":
            return segments
    elif 1 <= int(segments) <= SCAN_BWD_MAX_SEGMENTS:
        return int(segments)
    raise ValueError(f'segments must be an int in [1, {SCAN_BWD_MAX_SEGMENTS}] or "auto", got {segments!r}')


def _resolve_segments(segments, S: int, L: int, E: int, policy=scan_bwd_auto_segments) -> int:
    G = _check_segments(segments)
    return policy(S, L, E) if G == "auto" else G


def selective_scan_bwd(u, delta, A, B, C, D, z, delta_bias, dout, reverse=False, poison=False, segments=1, seg_entry=False):
    """pcad_selective_scan_bwd on selective_scan_fn's operands (upstream layouts; D, z, delta_bias may be None) and dout (B, E, L).
    -> namespace(du, ddelta, dz (B, E, L) in u's dtype (dz None without z); dB, dC fp32 (B, 16, L); dA fp32 (E, 16); dD, ddelta_bias fp32
    (E); guards_ok).  poison (tests): the scratch starts as 0xFF bytes and every output as NaN inside a larger buffer with one row of
    sentinels before and after it; guards_ok tells whether all sentinels are intact afterwards.
    segments: 1 is that entry (libpcad_train.so); 2..64 is pcad_selective_scan_bwd_seg (include/pcad_bwd.h, libpcad_bwd.so; DESIGN.md
    §4v), every strand cut into that many segments walked in parallel; "auto" resolves through scan_bwd_auto_segments.
    seg_entry (tests): the segmented entry even with segments == 1."""
    _require_gpu(u, "u")
    Bsz, E, L = u.shape
    dt, dev = u.dtype, u.device
    with torch.cuda.device(dev):
        G = _resolve_segments(segments, Bsz, L, E)
    seg = (G,) if G > 1 or seg_entry else ()
    lib, name = (load_bwd_library(), "pcad_selective_scan_bwd_seg") if seg else (load_train_library(), "pcad_selective_scan_bwd")
    u_tm, z_tm, bc, A32, Dv, db = _scan_common(u, B, C, A, D, z, delta_bias)
    d_tm = delta.to(dt).transpose(1, 2).contiguous()
    g_tm = dout.to(dt).transpose(1, 2).contiguous()
    f32 = torch.float32
    outs = [_guarded(sh, ty, dev, "row", poison) for sh, ty in (((Bsz, L, E), dt), ((Bsz, L, E), dt), ((Bsz, L, E), dt), ((Bsz, L, 32), f32),
                                                                ((E, 16), f32), ((E,), f32), ((E,), f32))]
    du, dd, dz, dbc, dA, dD, dbias = [o[0] for o in outs]
    if z_tm is None:
        dz = None
    nb = getattr(lib, name + "_scratch_bytes")(Bsz, L, E, *seg)
    scratch, scratch_ptr = _scratch(nb, dev, poison)
    with torch.cuda.device(dev):
        _check(getattr(lib, name)(u_tm.data_ptr(), d_tm.data_ptr(), _ptr(z_tm), E,
                                  bc.data_ptr(), A32.data_ptr(), Dv.data_ptr(), db.data_ptr(), g_tm.data_ptr(),
                                  du.data_ptr(), dd.data_ptr(), _ptr(dz), dbc.data_ptr(),
                                  dA.data_ptr(), dD.data_ptr(), dbias.data_ptr(), scratch_ptr, nb, Bsz, L, E,
                                  int(bool(reverse)), _dt(u_tm), *seg, _stream_ptr()), name)
    return SimpleNamespace(du=du.transpose(1, 2), ddelta=dd.transpose(1, 2), dz=dz.transpose(1, 2) if dz is not None else None,
                           dB=dbc[..., :16].transpose(1, 2), dC=dbc[..., 16:].transpose(1, 2), dA=dA, dD=dD, ddelta_bias=dbias,
                           guards_ok=_guards_intact(outs))


def selective_scan_fwd_seg(u, delta, A, B, C, D, z, delta_bias, reverse=False, segments=1, poison=False):
    """pcad_selective_scan_fwd_seg (include/pcad_bwd.h, libpcad_bwd.so) on selective_scan_fn's operands (upstream layouts; D,
    z, delta_bias may be None): the training forward's scan with every strand cut into `segments` segments (1..64 or "auto", resolved
    by scan_fwd_auto_segments) walked in parallel, on the backward's cut rule.  -> namespace(out (B, E, L) in u's dtype; segments: the
    resolved count; guards_ok).  segments == 1 runs this entry's own walk from a zero state - not pcad_selective_scan's bits, which is
    why selective_scan_fn never routes 1 here.  poison (tests): as selective_scan_bwd."""
    _require_gpu(u, "u")
    Bsz, E, L = u.shape
    dt, dev = u.dtype, u.device
    with torch.cuda.device(dev):
        G = _resolve_segments(segments, Bsz, L, E, scan_fwd_auto_segments)
    lib, name = load_bwd_library(), "pcad_selective_scan_fwd_seg"
    u_tm, z_tm, bc, A32, Dv, db = _scan_common(u, B, C, A, D, z, delta_bias)
    d_tm = delta.to(dt).transpose(1, 2).contiguous()
    outs = [_guarded((Bsz, L, E), dt, dev, "row", poison)]
    y = outs[0][0]
    nb = lib.pcad_selective_scan_fwd_seg_scratch_bytes(Bsz, L, E, G)
    scratch, scratch_ptr = _scratch(nb, dev, poison)
    with torch.cuda.device(dev):
        _check(lib.pcad_selective_scan_fwd_seg(u_tm.data_ptr(), d_tm.data_ptr(), _ptr(z_tm), E, bc.data_ptr(), A32.data_ptr(), Dv.data_ptr(),
                                               db.data_ptr(), y.data_ptr(), scratch_ptr, nb, Bsz, L, E, int(bool(reverse)), _dt(u_tm), G,
                                               _stream_ptr()), name)
    return SimpleNamespace(out=y.transpose(1, 2), segments=G, guards_ok=_guards_intact(outs))


CONV_BWD_SEG = 64        # csrc/kernels.hpp CONV_BWD_SEG: walk steps one lane of the conv backward owns (one row of dw | db partials each)
NORM_BWD_ROWS = 16       # csrc/kernels.hpp NORM_BWD_ROWS: consecutive rows one wave of the norm backward walks (one dweight partial row each)


def causal_conv1d_silu_bwd(x_tm, weight, bias, dout_tm, reverse=False, poison=False):
    """pcad_causal_conv1d_silu_bwd on causal_conv1d_dir's plain operands: x_tm [S, L, E] (a view whose rows are ldx >= E elements apart,
    such as the first half of a token-major xz, is read in place), weight (E, 4) or (E, 1, 4), bias (E), dout_tm [S, L, E].
    -> namespace(dx [S, L, E] in x's dtype; dw fp32 (E, 4); db fp32 (E); guards_ok).  poison (tests): as selective_scan_bwd."""
    _require_gpu(x_tm, "x")
    lib = load_bwd_library()
    S, L, E = x_tm.shape
    dt, dev = x_tm.dtype, x_tm.device
    ldx = x_tm.stride(1)
    in_place = (S * L > 0 and x_tm.stride(2) == 1 and x_tm.stride(0) == L * ldx and ldx >= E and (ldx * x_tm.element_size()) % 16 == 0
                and x_tm.data_ptr() % 16 == 0)
    if not in_place:
        x_tm, ldx = x_tm.contiguous(), E
    w = weight.reshape(E, -1).float().contiguous()
    b = bias.float().contiguous()
    g = dout_tm.to(dt).contiguous()
    f32 = torch.float32
    outs = [_guarded(sh, ty, dev, "row", poison) for sh, ty in (((S, L, E), dt), ((E, 4), f32), ((E,), f32))]
    dx, dw, db = [o[0] for o in outs]
    nb = lib.pcad_causal_conv1d_silu_bwd_scratch_bytes(S, L, E)
    scratch, scratch_ptr = _scratch(nb, dev, poison)
    with torch.cuda.device(dev):
        _check(lib.pcad_causal_conv1d_silu_bwd(x_tm.data_ptr(), ldx, w.data_ptr(), b.data_ptr(), g.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                               db.data_ptr(), scratch_ptr, nb, S, L, E, int(bool(reverse)), _dt(x_tm), _stream_ptr()),
               "pcad_causal_conv1d_silu_bwd")
    return SimpleNamespace(dx=dx, dw=dw, db=db, guards_ok=_guards_intact(outs))


def add_rmsnorm_bwd(x, residual, weight, dy, dresidual_out, eps, residual_in_fp32, poison=False):
    """pcad_add_rmsnorm_bwd on rms_norm_fn's operands: x, dy [..., D]; residual [..., D] or None; dresidual_out [..., D] (the gradient
    of the prenorm output) or None.  The residual tensors are taken in the residual dtype (fp32 with residual_in_fp32 or an fp32 x,
    else x's).  -> namespace(dx like x; dresidual_in like x in the residual dtype, None without residual; dweight fp32 (D); guards_ok).
    poison (tests): as selective_scan_bwd."""
    _require_gpu(x, "x")
    lib = load_bwd_library()
    D = x.shape[-1]
    dt, dev = x.dtype, x.device
    rdt = _residual_dtype(dt, residual_in_fp32)
    xf = x.contiguous().view(-1, D)
    rows = xf.shape[0]
    res = residual.to(rdt).contiguous().view(-1, D) if residual is not None else None
    g = dy.to(dt).contiguous().view(-1, D)
    gres = dresidual_out.to(rdt).contiguous().view(-1, D) if dresidual_out is not None else None
    w = weight.float().contiguous()
    outs = [_guarded(sh, ty, dev, "row", poison) for sh, ty in (((rows, D), dt), ((rows, D), rdt), ((D,), torch.float32))]
    dx, dres, dw = [o[0] for o in outs]
    if res is None:
        dres, outs[1] = None, (outs[1][0], None)
    nb = lib.pcad_add_rmsnorm_bwd_scratch_bytes(rows, D)
    scratch, scratch_ptr = _scratch(nb, dev, poison)
    with torch.cuda.device(dev):
        _check(lib.pcad_add_rmsnorm_bwd(xf.data_ptr(), _ptr(res), w.data_ptr(), g.data_ptr(), _ptr(gres), dx.data_ptr(), _ptr(dres), dw.data_ptr(),
                                        scratch_ptr, nb, rows, D, float(eps), _dt(xf), _DT[rdt], _stream_ptr()), "pcad_add_rmsnorm_bwd")
    return SimpleNamespace(dx=dx.view(x.shape), dresidual_in=dres.view(x.shape) if dres is not None else None, dweight=dw,
                           guards_ok=_guards_intact(outs))


class _CausalConv1dDirFn(torch.autograd.Function):
    """causal_conv1d_dir (plain rows) with a backward: pcad_causal_conv1d_silu_bwd (include/pcad_bwd.h, libpcad_bwd.so).  weight (E, 4) and
    bias (E) arrive in fp32 (the casts are torch ops outside).  Only the inputs are saved; the kernel recomputes the pre-activation."""

    @staticmethod
    def forward(ctx, x_tm, weight, bias, reverse):
        ctx.save_for_backward(x_tm, weight, bias)
        ctx.reverse = bool(reverse)
        return _causal_conv1d_dir_forward(x_tm, weight, bias, reverse, False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x_tm, weight, bias = ctx.saved_tensors
        g = causal_conv1d_silu_bwd(x_tm, weight, bias, dout, ctx.reverse)
        need = ctx.needs_input_grad
        return g.dx if need[0] else None, g.dw if need[1] else None, g.db if need[2] else None, None


class _RmsNormFn(torch.autograd.Function):
    """rms_norm_fn (always with the prenorm output) with a backward: pcad_add_rmsnorm_bwd (include/pcad_bwd.h, libpcad_bwd.so).  weight
    arrives in fp32 and residual in the residual dtype.  Only the inputs are saved; the kernel recomputes rstd."""

    @staticmethod
    def forward(ctx, x, weight, residual, eps, residual_in_fp32):
        ctx.save_for_backward(x, weight, residual)
        ctx.eps, ctx.res_fp32 = eps, residual_in_fp32
        ctx.set_materialize_grads(False)              # an output nobody used arrives as None, not as a tensor of zeros
        return _rms_norm_forward(x, weight, residual, eps, True, residual_in_fp32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, dres_out):
        x, weight, residual = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(x)
        g = add_rmsnorm_bwd(x, residual, weight, dy, dres_out, ctx.eps, ctx.res_fp32)
        need = ctx.needs_input_grad
        return (g.dx if need[0] else None, g.dweight if need[1] else None,
                g.dresidual_in if residual is not None and need[2] else None, None, None)


class _SelectiveScanFn(torch.autograd.Function):
    """selective_scan_fn with a backward: the forward is the plain call - with fwd_segments > 1 pcad_selective_scan_fwd_seg (include/pcad_bwd.h;
    DESIGN.md §4w) -, the backward pcad_selective_scan_bwd (include/pcad_train.h, libpcad_train.so) or, with segments > 1,
    pcad_selective_scan_bwd_seg (include/pcad_bwd.h, libpcad_bwd.so).  Only the inputs are saved; the kernel recomputes the states."""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, z, delta_bias, reverse, segments=1, fwd_segments=1):
        ctx.save_for_backward(u, delta, A, B, C, D, z, delta_bias)
        ctx.reverse = bool(reverse)
        ctx.segments = segments
        ctx.fwd_segments = fwd_segments
        return _selective_scan_forward(u, delta, A, B, C, D, z, delta_bias, reverse, None, False, fwd_segments)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        u, delta, A, B, C, D, z, delta_bias = ctx.saved_tensors
        g = selective_scan_bwd(u, delta, A, B, C, D, z, delta_bias, dout, ctx.reverse, segments=ctx.segments)
        need = ctx.needs_input_grad
        return (g.du if need[0] else None,
                g.ddelta.to(delta.dtype) if need[1] else None,
                g.dA.to(A.dtype) if need[2] else None,
                g.dB.to(B.dtype) if need[3] else None,
                g.dC.to(C.dtype) if need[4] else None,
                g.dD.to(D.dtype) if D is not None and need[5] else None,
                g.dz.to(z.dtype) if z is not None and need[6] else None,
                g.ddelta_bias.to(delta_bias.dtype) if delta_bias is not None and need[7] else None,
                None, None, None)


def selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False,
                      return_last_state=False, reverse=False, accumulate_into=None, gate_sum=False, segments=1, fwd_segments=1):
    """u, delta, z: (B, E, L); A: (E, 16); B, C: (B, 16, L); D, delta_bias: (E).  Returns (B, E, L).
    accumulate_into: add this call's gated output to an earlier one (bi-directional "add"); with gate_sum=True the
    earlier output is taken as UNGATED (its call had z=None) and SiLU(z) is applied once to the sum (the engine's form).
    When any of u, delta, A, B, C, D, z, delta_bias requires grad the call is differentiable (pcad_selective_scan_bwd; either
    direction): each gradient comes back in its input's shape and dtype.  accumulate_into / gate_sum are inference forms and are
    refused then - the bidirectional sum is two calls added in torch.
    segments (1, 2..64 or "auto"; selective_scan_bwd): how many segments the BACKWARD cuts every strand into; the forward is the same
    call, and the same bits, whatever it is.
    fwd_segments (1, 2..64 or "auto": scan_fwd_auto_segments, the backward's policy cut back where few segments fill the device): how many segments the FORWARD cuts every strand into, with or without
    grad.  Resolved to 1 it is today's pcad_selective_scan call, bit for bit; above 1 it is pcad_selective_scan_fwd_seg,
    whose result differs by fp32 rounding and is bit-reproducible for a given count.  Not with accumulate_into / gate_sum."""
    _require_gpu(u, "u")
    segments = _check_segments(segments)
    fwd_segments = _check_segments(fwd_segments)
    if not delta_softplus:
        raise NotImplementedError("the Caduceus path always uses delta_softplus=True")
    if return_last_state:
        raise NotImplementedError("return_last_state is not on the Caduceus path")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (u, delta, A, B, C, D, z, delta_bias)):
        if accumulate_into is not None or gate_sum:
            raise NotImplementedError("accumulate_into / gate_sum are inference forms: with an input that requires grad, add the "
                                      "two directions' outputs in torch")
        return _SelectiveScanFn.apply(u, delta, A, B, C, D, z, delta_bias, reverse, segments, fwd_segments)
    return _selective_scan_forward(u, delta, A, B, C, D, z, delta_bias, reverse, accumulate_into, gate_sum, fwd_segments)


def _selective_scan_forward(u, delta, A, B, C, D, z, delta_bias, reverse, accumulate_into, gate_sum, fwd_segments=1):
    Bsz, E, L = u.shape
    if fwd_segments != 1:
        if accumulate_into is not None or gate_sum:               # whatever "auto" would resolve to: the refusal does not depend on the shape
            raise NotImplementedError("accumulate_into / gate_sum are not built for the segmented forward (fwd_segments other than 1)")
        with torch.cuda.device(u.device):
            G = _resolve_segments(fwd_segments, Bsz, L, E, scan_fwd_auto_segments)
        if G > 1 and L > scan_bwd_seg_steps(L, G):                # one effective segment: today's call, and its bits
            return selective_scan_fwd_seg(u, delta, A, B, C, D, z, delta_bias, reverse, G).out
    lib = load_library()
    u_tm, z_tm, bc, A32, Dv, db = _scan_common(u, B, C, A, D, z, delta_bias)
    d_tm = delta.to(u.dtype).transpose(1, 2).contiguous()
    y = accumulate_into.transpose(1, 2).contiguous() if accumulate_into is not None else torch.empty_like(u_tm)
    with torch.cuda.device(u.device):
        _check(lib.pcad_selective_scan(u_tm.data_ptr(), d_tm.data_ptr(), _ptr(z_tm), E, bc.data_ptr(), A32.data_ptr(), Dv.data_ptr(),
                                       db.data_ptr(), y.data_ptr(), Bsz, L, E, int(bool(reverse)), _acc_mode(accumulate_into, gate_sum),
                                       _dt(u_tm), _stream_ptr()), "pcad_selective_scan")
    return y.transpose(1, 2)


def selective_scan_dtproj_fn(u, dt_low, dt_proj_weight, A, B, C, D=None, z=None, delta_bias=None, reverse=False,
                             accumulate_into=None, gate_sum=False):
    """mamba_inner_fn's tail: delta = dt_proj_weight @ dt_low (on MFMA inside the kernel), then selective_scan_fn.
    u, z: (B, E, L); dt_low: (B, L, R); dt_proj_weight: (E, R)."""
    _require_gpu(u, "u")
    Bsz, E, L = u.shape
    u_tm, z_tm, bc, A32, Dv, db = _scan_common(u, B, C, A, D, z, delta_bias)
    y = accumulate_into.transpose(1, 2).contiguous() if accumulate_into is not None else torch.empty_like(u_tm)
    _scan_dtproj(u_tm, dt_low, dt_low.shape[-1], dt_proj_weight, z_tm, bc, A32, Dv, db, y, Bsz, L, reverse, _acc_mode(accumulate_into, gate_sum))
    return y.transpose(1, 2)


def _pad_cols(t, R: int, cols: int, dtype, dev):
    """t [..., R] -> [..., cols] in `dtype`, zeros behind column R"""
    p = torch.zeros((*t.shape[:-1], cols), dtype=dtype, device=dev)
    p[..., :R] = t.to(dtype)
    return p


def _scan_dtproj(u_tm, dt_low, R, dt_proj_weight, z_tm, bc, A32, Dv, db, y, Bsz, L, reverse, acc):
    """pcad_selective_scan_dtproj into y: u_tm, y [B * L, E] rows (z_tm likewise, or None); dt_low [..., R] and dt_proj_weight (E, R) are
    zero padded here to padded_dt_rank(R) columns in u's dtype - a dt_low that arrives that wide (the fused conv + x_proj's) is taken as
    it is; bc, A32, Dv, db as `_scan_common` makes them; acc: `_acc_mode`."""
    lib = load_library()
    E, dt, dev = u_tm.shape[-1], u_tm.dtype, u_tm.device
    Rp = padded_dt_rank(R)
    dl = dt_low.to(dt).contiguous() if dt_low.shape[-1] == Rp else _pad_cols(dt_low, R, Rp, dt, dev)
    W = _pad_cols(dt_proj_weight, R, Rp, dt, dev)
    with torch.cuda.device(dev):
        _check(lib.pcad_selective_scan_dtproj(u_tm.data_ptr(), dl.data_ptr(), Rp, W.data_ptr(), Rp, _ptr(z_tm), E, bc.data_ptr(),
                                              A32.data_ptr(), Dv.data_ptr(), db.data_ptr(), y.data_ptr(), Bsz, L, E,
                                              int(bool(reverse)), acc, _dt(u_tm), _stream_ptr()), "pcad_selective_scan_dtproj")


def mamba_inner_fn(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias,
                   A, B=None, C=None, D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True,
                   reverse=False, scan_bwd_segments=1, scan_fwd_segments=1):
    """`mamba_ssm.ops.selective_scan_interface.mamba_inner_fn` (mamba-ssm 2.2.2, reference env/requirements.txt:10) - the ONE call
    `Mamba.forward`'s fast path makes after in_proj - under its own signature, on the engine's kernels:

        x, z    = xz.chunk(2, dim=1)                                        xz (B, 2E, L) channels-first, as upstream
        xc      = causal_conv1d_fn(x, conv1d_weight, conv1d_bias, "silu")   \  pcad_conv_xproj_bidir (one kernel; dt_rank <= 96),
        x_dbl   = F.linear(xc^T, x_proj_weight)          (R + 2N columns)   /  else pcad_causal_conv1d_silu + pcad_gemm_nt
        delta   = delta_proj_weight @ x_dbl[:, :R]^T                        \  pcad_selective_scan_dtproj (dt_proj on MFMA inside
        y       = selective_scan_fn(xc, delta, A, B_t, C_t, D, z, delta_bias, delta_softplus=True)   /  the scan; delta never stored)
        return    F.linear(y^T, out_proj_weight)                               pcad_gemm_nt            -> (B, L, D)

    conv1d_weight (E, 1, 4) or (E, 4); x_proj_weight (R + 32, E); delta_proj_weight (E, R); out_proj_weight (D, E);
    A (E, 16) = -exp(A_log) as upstream passes it; D, delta_bias (E).  B / C must be None (input-dependent, taken from x_dbl - the only
    form Mamba.forward uses), likewise the projection biases and out_proj_bias (Caduceus builds Mamba with bias=False).
    reverse=True is the twin BiMambaWrapper needs for `mamba_rev`: the same operator walking right-to-left with the anti-causal
    conv on the SAME rows, i.e. mamba_inner_fn(xz, ..., reverse=True) == mamba_inner_fn(xz.flip(-1), ...).flip(1) without either
    flip copy.  Tensors are ROCm tensors in one dtype (fp32 or bf16); parameters are converted as the engine's
    weight packing does (conv taps, A, D, biases to fp32; projections to xz.dtype).

    With grad mode on and any tensor input requiring grad the call takes a composed path of the differentiable operators, chained by
    torch autograd: causal_conv1d_dir (pcad_causal_conv1d_silu_bwd), F.linear for x_proj, dt_proj and out_proj (differentiated by stock
    PyTorch-ROCm), selective_scan_fn (pcad_selective_scan_bwd).  That path stores xc, x_dbl, delta and y in the model dtype - upstream's
    own rounding points - so its forward value agrees with the fused inference path within test_mamba_inner_fn's bars (3e-5 fp32,
    2^-7 bf16 against the oracle), not bit for bit.  With nothing requiring grad the function is unchanged.
    scan_bwd_segments goes to selective_scan_fn's `segments` on that path (the scan's backward only; no forward bit changes), and
    scan_fwd_segments to its `fwd_segments` (the scan's forward in segments; 1: no bit changes).  Both are read on the
    grad path only."""
    _require_gpu(xz, "xz")
    if B is not None or C is not None:
        raise NotImplementedError("constant B / C are not on the Caduceus path (Mamba.forward passes None: input-dependent B, C)")
    if out_proj_bias is not None or B_proj_bias is not None or C_proj_bias is not None:
        raise NotImplementedError("projection biases are not on the Caduceus path (Mamba(bias=False))")
    if not delta_softplus:
        raise NotImplementedError("the Caduceus path always uses delta_softplus=True")
    load_library()
    Bsz, E2, L = xz.shape
    E = E2 // 2
    dt, dev = xz.dtype, xz.device
    if A.shape != (E, 16):
        raise ValueError(f"A must be (d_inner, 16), got {tuple(A.shape)}")
    R = delta_proj_weight.shape[1]
    if x_proj_weight.shape != (R + 32, E):
        raise ValueError(f"x_proj_weight must be (dt_rank + 2 * 16, d_inner) = ({R + 32}, {E}), got {tuple(x_proj_weight.shape)}")
    w = conv1d_weight.reshape(E, -1)
    if w.shape[1] != 4:
        raise NotImplementedError("only conv width 4")
    bias = conv1d_bias if conv1d_bias is not None else torch.zeros(E, device=dev)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight,
                                                                                  out_proj_weight, A, D, delta_bias)):
        xc = causal_conv1d_dir(xz[:, :E].transpose(1, 2), w, bias, reverse)                      # (B, L, E)
        # linear_fn: F.linear(x, weight.to(dt)) itself unless the weight carries an fp32 main_grad
        x_dbl = linear_fn(xc, x_proj_weight)                                                     # (B, L, R + 32)
        delta = linear_fn(x_dbl[..., :R], delta_proj_weight).transpose(1, 2)                     # (B, E, L)
        y = selective_scan_fn(xc.transpose(1, 2), delta, A, x_dbl[..., R:R + 16].transpose(1, 2), x_dbl[..., R + 16:].transpose(1, 2), D,
                              z=xz[:, E:], delta_bias=delta_bias, delta_softplus=True, reverse=reverse, segments=scan_bwd_segments,
                              fwd_segments=scan_fwd_segments)
        return linear_fn(y.transpose(1, 2), out_proj_weight)
    x_tm = xz[:, :E].transpose(1, 2).contiguous()                    # the engine is token-major (test plumbing: it never transposes)
    z_tm = xz[:, E:].transpose(1, 2).contiguous()
    rows = Bsz * L
    d = 1 if reverse else 0
    fused = R <= 96 and (E * xz.element_size()) % 128 == 0 and (rows + 16) * E * xz.element_size() < 2 ** 32
    if fused:
        xc_b, dtl, bc, _, _ = _conv_xproj_raw(x_tm, w, bias, w, bias, x_proj_weight, x_proj_weight)
        xc = from_blocked(xc_b[d], rows)
        dl, bcd = dtl[d], bc[d]                                      # dt_low already padded_dt_rank(R) wide
    else:
        yf, yr = causal_conv1d_bidir(x_tm, w, bias, w, bias)
        xc = (yr if reverse else yf).reshape(rows, E)
        x_dbl = linear(xc, x_proj_weight)                            # [rows, R + 32] in xz.dtype (rounded like upstream's F.linear)
        dl, bcd = x_dbl[:, :R], x_dbl[:, R:].float().contiguous()
    y = torch.empty((rows, E), dtype=dt, device=dev)
    _scan_dtproj(xc, dl, R, delta_proj_weight, z_tm, bcd, *_scan_params(A, D, delta_bias, E, dev), y, Bsz, L, reverse, 0)
    return linear(y.view(Bsz, L, E), out_proj_weight)


def linear(x, weight, out_dtype: Optional[torch.dtype] = None):
    """F.linear(x, weight) on MFMA: x [..., K], weight [N, K] (same dtype), K*elem a multiple of 128 bytes."""
    _require_gpu(x, "x")
    lib = load_library()
    K = x.shape[-1]
    N = weight.shape[0]
    xf = x.contiguous().view(-1, K)
    wf = weight.to(x.dtype).contiguous()
    od = out_dtype or x.dtype
    out = torch.empty((xf.shape[0], N), dtype=od, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib.pcad_gemm_nt(xf.data_ptr(), K, wf.data_ptr(), K, out.data_ptr(), N, xf.shape[0], N, K, _dt(xf),
                                _DT[od], _stream_ptr()), "pcad_gemm_nt")
    return out.view(*x.shape[:-1], N)


def linear_split(x, weight):
    """F.linear(x, weight) of fp32 tensors as ONE split-bf16 GEMM on the bf16 matrix pipes (include/pcad.h pcad_gemm_nt_split):
    x [..., K], weight [N, K], K % 64 == 0 -> fp32 [..., N]."""
    _require_gpu(x, "x")
    lib = load_library()
    if x.dtype != torch.float32:
        raise ValueError("linear_split takes fp32 tensors")
    K = x.shape[-1]
    N = weight.shape[0]
    xf = x.contiguous().view(-1, K)
    wf = weight.float().contiguous()
    M = xf.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    nb = lib.pcad_gemm_nt_split_scratch_bytes(M, N, K)
    scratch, scratch_ptr = _scratch(nb, x.device)
    with torch.cuda.device(x.device):
        _check(lib.pcad_gemm_nt_split(xf.data_ptr(), K, wf.data_ptr(), K, out.data_ptr(), N, M, N, K, scratch_ptr, nb, _stream_ptr()),
               "pcad_gemm_nt_split")
    return out.view(*x.shape[:-1], N)


def to_res_fragment(res: torch.Tensor) -> torch.Tensor:
    """[M, N] (M, N multiples of 256) -> the same values in the 4-wave GEMM's fragment layout (include/pcad.h
    pcad_gemm_nt_residual), as a flat [M * N] tensor."""
    M, N = res.shape
    if M % 256 or N % 256:
        raise ValueError("the fragment layout needs M % 256 == 0 and N % 256 == 0")
    #          tm        wm i  li   tn        wn jg lg k  r
    v = res.reshape(M // 256, 2, 8, 16, N // 256, 2, 2, 4, 4, 4)
    #  -> [tm, tn, wm, wn, i, jg, k, lg, li, r]
    return v.permute(0, 4, 1, 5, 2, 6, 8, 7, 3, 9).contiguous().view(-1)


def from_res_fragment(frag: torch.Tensor, M: int, N: int) -> torch.Tensor:
    v = frag.view(M // 256, N // 256, 2, 2, 8, 2, 4, 4, 16, 4)
    #  [tm, tn, wm, wn, i, jg, k, lg, li, r] -> [tm, wm, i, li, tn, wn, jg, lg, k, r]
    return v.permute(0, 2, 4, 8, 1, 3, 5, 7, 6, 9).contiguous().view(M, N)


def linear_residual(x, weight, residual):
    """The "norm_fold" out_proj as an operator (include/pcad.h pcad_gemm_nt_residual): residual fp32 [M, N] + x [M, K] @ weight
    [N, K]^T.  Returns (new residual fp32 [M, N], round(new residual) in x.dtype [M, N], ssq [M, N/128] per-row partial sums of
    squares).  The kernel updates the residual in place in its fragment layout; the conversions are done here (test plumbing)."""
    _require_gpu(x, "x")
    lib = load_library()
    M, K = x.shape
    N = weight.shape[0]
    if M % 256 or N % 256:
        raise RuntimeError("pcad_gemm_nt_residual: M and N must be multiples of 256")
    if residual.dtype != torch.float32 or tuple(residual.shape) != (M, N):
        raise ValueError("residual must be an fp32 [M, N] tensor")
    xf = x.contiguous()
    wf = weight.to(x.dtype).contiguous()
    frag = to_res_fragment(residual)
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    ssq = torch.empty((M, N // 128), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib.pcad_gemm_nt_residual(xf.data_ptr(), K, wf.data_ptr(), K, out.data_ptr(), frag.data_ptr(), ssq.data_ptr(),
                                         M, N, K, _dt(xf), _stream_ptr()), "pcad_gemm_nt_residual")
    return from_res_fragment(frag, M, N), out, ssq


# ---- the engine's GEMM launch forms as operators (include/pcad.h "Engine forms of the GEMMs") ----------------------------------------
# Layout conversion only (to_blocked / from_blocked, the residual's fragment layout): the operands are taken as the caller built them,
# split [hi | lo] forms included.  Every output - `rows` rows of `width` elements, plain or blocked: the kernel's business - starts as
# NaN between two guards of whole lines (`_guarded`, geometry "lines").
def _gemm_a(a: torch.Tensor, a_blocked: bool, lda_extra: int):
    """A as a launch takes it: blocked (padding rows NaN), or plain rows with lda_extra NaN columns behind each.  -> (tensor, lda)"""
    a = a.contiguous()
    if a_blocked:
        if lda_extra:
            raise ValueError("a blocked A has rows of exactly its own width")
        return to_blocked(a, pad_value=float("nan")), a.shape[1]
    if lda_extra:
        buf = torch.full((a.shape[0], a.shape[1] + lda_extra), float("nan"), dtype=a.dtype, device=a.device)
        buf[:, :a.shape[1]] = a
        return buf, buf.shape[1]
    return a, a.shape[1]


def _unblock(out: torch.Tensor, rows: int):
    """a blocked output buffer [rows8, width] -> (its `rows` rows as plain rows, its padding rows)"""
    rows8, width = out.shape
    per = 128 // out.element_size()
    return _split_blocked(out.view(rows8 // 8, width // per, 8, per), rows)


def gemm_nt_engine(a, w, K: Optional[int] = None, a_blocked: bool = False, ksplit: int = 0, out_dtype: Optional[torch.dtype] = None,
                   lda_extra: int = 0):
    """pcad_gemm_nt_engine (the engine's out_proj launch): a [M, K] - or, ksplit = Ko / 64, bf16 [M, 2 Ko] = [hi | lo] with K = 3 Ko -,
    w [N, K] (or [N, 2 Ko]); a_blocked: A goes through the blocked layout.  -> namespace(c [M, N] out_dtype, guards_ok)."""
    _require_gpu(a, "a")
    lib = load_library()
    M, N = a.shape[0], w.shape[0]
    K = a.shape[1] if K is None else K
    od = out_dtype or a.dtype
    ab, lda = _gemm_a(a, a_blocked, lda_extra)
    wf = w.contiguous()
    c = _guarded((M, N), od, a.device, "lines")
    with torch.cuda.device(a.device):
        _check(lib.pcad_gemm_nt_engine(ab.data_ptr(), lda, wf.data_ptr(), wf.shape[1], c[0].data_ptr(), N, M, N, K, int(bool(a_blocked)),
                                       int(ksplit), _dt(a), _DT[od], _stream_ptr()), "pcad_gemm_nt_engine")
    return SimpleNamespace(c=c[0], guards_ok=_guards_intact([c]))


def gemm_nt_xproj(a, w, nsplit: int, a_blocked: bool = False, ksplit: int = 0):
    """pcad_gemm_nt_xproj (the engine's x_proj launch where the fused conv + x_proj kernel is off): a [M, K], w [N, K] ->
    namespace(c [M, nsplit] in a's dtype, c2 fp32 [M, N - nsplit] holding values rounded to a's dtype, guards_ok)."""
    _require_gpu(a, "a")
    lib = load_library()
    M, N, K = a.shape[0], w.shape[0], a.shape[1]
    ab, lda = _gemm_a(a, a_blocked, 0)
    wf = w.contiguous()
    c = _guarded((M, nsplit), a.dtype, a.device, "lines")
    c2 = _guarded((M, N - nsplit), torch.float32, a.device, "lines")
    with torch.cuda.device(a.device):
        _check(lib.pcad_gemm_nt_xproj(ab.data_ptr(), lda, wf.data_ptr(), wf.shape[1], c[0].data_ptr(), nsplit, c2[0].data_ptr(), N - nsplit,
                                      nsplit, M, N, K, int(bool(a_blocked)), int(ksplit), _dt(a), _stream_ptr()), "pcad_gemm_nt_xproj")
    return SimpleNamespace(c=c[0], c2=c2[0], guards_ok=_guards_intact([c, c2]))


def gemm_nt_two(a, w, nsplit: int, K: Optional[int] = None, out_blocked: bool = False, rscale=None, ksplit: int = 0,
                out_dtype: Optional[torch.dtype] = None, lda_extra: int = 0, a_blocked: bool = False):
    """pcad_gemm_nt_two (the engine's in_proj launch): a, w, K, ksplit, lda_extra as in gemm_nt_engine; rscale fp32 [M] or None.
    out_blocked: both outputs go through the blocked layout.  a_blocked is refused by the library (the form has none).
    -> namespace(c1 [M, nsplit], c2 [M, N - nsplit] out_dtype; pad1, pad2: the blocked buffers' padding rows (empty for plain
    outputs); guards_ok)."""
    _require_gpu(a, "a")
    lib = load_library()
    M, N = a.shape[0], w.shape[0]
    K = a.shape[1] if K is None else K
    od = out_dtype or a.dtype
    ab, lda = _gemm_a(a, a_blocked, lda_extra)
    wf = w.contiguous()
    rs = rscale.float().contiguous() if rscale is not None else None
    rows = _round_up(M, 8) if out_blocked else M
    c1, c2 = _guarded((rows, nsplit), od, a.device, "lines"), _guarded((rows, N - nsplit), od, a.device, "lines")
    with torch.cuda.device(a.device):
        _check(lib.pcad_gemm_nt_two(ab.data_ptr(), lda, wf.data_ptr(), wf.shape[1], c1[0].data_ptr(), c2[0].data_ptr(), nsplit,
                                    _ptr(rs), M, N, K, int(bool(a_blocked)), int(bool(out_blocked)),
                                    int(ksplit), _dt(a), _DT[od], _stream_ptr()), "pcad_gemm_nt_two")
    if out_blocked:
        (o1, p1), (o2, p2) = _unblock(c1[0], M), _unblock(c2[0], M)
    else:
        (o1, p1), (o2, p2) = (c1[0], c1[0][M:]), (c2[0], c2[0][M:])
    return SimpleNamespace(c1=o1, c2=o2, pad1=p1, pad2=p2, guards_ok=_guards_intact([c1, c2]))


def gemm_nt_residual_engine(a, w, residual, a_blocked: bool = False, ksplit: int = 0):
    """pcad_gemm_nt_residual_engine: `linear_residual` with A through the blocked layout (the engine's "norm_fold" out_proj launch).
    -> namespace(res fp32 [M, N], c [M, N] in a's dtype, ssq fp32 [M, N / 128], guards_ok)."""
    _require_gpu(a, "a")
    lib = load_library()
    M, K = a.shape
    N = w.shape[0]
    if residual.dtype != torch.float32 or tuple(residual.shape) != (M, N):
        raise ValueError("residual must be an fp32 [M, N] tensor")
    ab, lda = _gemm_a(a, a_blocked, 0)
    wf = w.contiguous()
    res = _guarded((M, N), torch.float32, a.device, "lines")
    res[0].view(-1).copy_(to_res_fragment(residual))
    c, ssq = _guarded((M, N), a.dtype, a.device, "lines"), _guarded((M, N // 128), torch.float32, a.device, "lines")
    with torch.cuda.device(a.device):
        _check(lib.pcad_gemm_nt_residual_engine(ab.data_ptr(), lda, wf.data_ptr(), wf.shape[1], c[0].data_ptr(), res[0].data_ptr(),
                                                ssq[0].data_ptr(), M, N, K, int(bool(a_blocked)), int(ksplit), _dt(a), _stream_ptr()),
               "pcad_gemm_nt_residual_engine")
    return SimpleNamespace(res=from_res_fragment(res[0].view(-1), M, N), c=c[0], ssq=ssq[0], guards_ok=_guards_intact([res, c, ssq]))


def gather_rows(src, B: int, L: int, positions):
    """src [2B*L, E] -> [2B*P, E]: strand b row p_q, strand B+b row L-1-p_q (include/pcad.h pcad_gather_rows)."""
    _require_gpu(src, "src")
    lib = load_library()
    E = src.shape[-1]
    P = len(positions)
    srcf = src.contiguous()
    out = torch.empty((2 * B * P, E), dtype=src.dtype, device=src.device)
    arr = (C.c_int32 * max(P, 1))(*[int(p) for p in positions])
    with torch.cuda.device(src.device):
        _check(lib.pcad_gather_rows(srcf.data_ptr(), out.data_ptr(), B, L, E, arr, P, _dt(srcf), _stream_ptr()), "pcad_gather_rows")
    return out


def final_head(h, res, norm_weight, emb, complement, B: int, L: int, eps: float, positions=None, pos_per_seq=None,
               h_compact: bool = False, want_hidden: bool = True, want_logits: bool = True, ids=None, status=None,
               res_fragment: bool = False):
    """norm_f + RC re-assembly + tied RCPS LM head at the requested positions (include/pcad.h pcad_final_head).
    h [2B*L, D] (or the gathered rows when h_compact), res [2B*L, D] (fp32 or h.dtype), emb [V, D] (rounded to h.dtype here, as the
    tied lm_head weight is).  -> (hidden [B, Q, 2D] | None, logits fp32 [B, Q, V] | None)."""
    _require_gpu(h, "h")
    lib = load_library()
    D = h.shape[-1]
    V = emb.shape[0]
    P = 0 if positions is None else len(positions)
    Q = 1 if pos_per_seq is not None else (P if P else L)
    hf, rf = h.contiguous(), res.contiguous()
    w = norm_weight.float().contiguous()
    e32 = emb.to(h.dtype).float().contiguous()
    comp = torch.as_tensor(list(complement), dtype=torch.int32, device=h.device)
    hid = torch.empty((B, Q, 2 * D), dtype=h.dtype, device=h.device) if want_hidden else None
    lg = torch.empty((B, Q, V), dtype=torch.float32, device=h.device) if want_logits else None
    arr = (C.c_int32 * max(P, 1))(*[int(p) for p in (positions or [])]) if P else None
    pps = pos_per_seq.to(torch.int32).contiguous() if pos_per_seq is not None else None
    with torch.cuda.device(h.device):
        _check(lib.pcad_final_head(hf.data_ptr(), rf.data_ptr(), w.data_ptr(), e32.data_ptr(), comp.data_ptr(),
                                   _ptr(hid), _ptr(lg),
                                   B, L, D, float(eps), arr, P, _ptr(pps), int(bool(h_compact)),
                                   _ptr(ids), _ptr(status),
                                   _dt(hf), _DT[rf.dtype], int(bool(res_fragment)), _stream_ptr()), "pcad_final_head")
    return hid, lg


def probs_head(h, res, norm_weight, emb, complement, cols, B: int, L: int, eps: float, positions=None, positions_per_window=None,
               h_compact: bool = False, want_probs: bool = True, want_logits: bool = False, ids=None, status=None,
               res_fragment: bool = False):
    """norm_f + tied RCPS LM head + fp32 softmax over the four vocabulary columns `cols`, at the requested positions
    (include/pcad.h pcad_probs_head).  h / res / emb / ids / status as in `final_head`; positions: None (all L) or a shared list;
    positions_per_window: integer tensor [B, P] on h's device (exclusive with positions).
    -> (probs fp32 [B, Q, 4] | None, logits fp32 [B, Q, V] | None)."""
    _require_gpu(h, "h")
    lib = load_library()
    D = h.shape[-1]
    V = emb.shape[0]
    ppw = positions_per_window.to(torch.int32).contiguous() if positions_per_window is not None else None
    P = int(ppw.shape[1]) if ppw is not None else (0 if positions is None else len(positions))
    Q = P if P else L
    hf, rf = h.contiguous(), res.contiguous()
    w = norm_weight.float().contiguous()
    e32 = emb.to(h.dtype).float().contiguous()
    comp = torch.as_tensor(list(complement), dtype=torch.int32, device=h.device)
    pr = torch.empty((B, Q, 4), dtype=torch.float32, device=h.device) if want_probs else None
    lg = torch.empty((B, Q, V), dtype=torch.float32, device=h.device) if want_logits else None
    arr = (C.c_int32 * P)(*[int(p) for p in positions]) if positions is not None and len(positions) else None
    with torch.cuda.device(h.device):
        _check(lib.pcad_probs_head(hf.data_ptr(), rf.data_ptr(), w.data_ptr(), e32.data_ptr(), comp.data_ptr(),
                                   (C.c_int32 * 4)(*[int(c) for c in cols]), _ptr(pr),
                                   _ptr(lg), B, L, D, float(eps), arr, P,
                                   _ptr(ppw), int(bool(h_compact)),
                                   _ptr(ids), _ptr(status),
                                   _dt(hf), _DT[rf.dtype], int(bool(res_fragment)), _stream_ptr()), "pcad_probs_head")
    return pr, lg


def layer_rows(src, B: int, L: int, positions=None, positions_per_window=None, assembled: bool = False, average: bool = False,
               status=None):
    """One level of hidden_states at the evaluated positions (include/pcad.h pcad_layer_rows).  src [2B*L, D] plain rows (a mixer
    output / the RCPS embedding), or - assembled - [B, P, 2D] rows already in hidden_states' layout; positions: a shared list, or
    positions_per_window: integer tensor [B, P] on src's device (exactly one).  -> [B, P, 2D] in src's dtype, or - average - the
    strand-averaged fp32 [B, P, D]."""
    _require_gpu(src, "src")
    lib = load_library()
    D = src.shape[-1] // 2 if assembled else src.shape[-1]
    ppw = positions_per_window.to(torch.int32).contiguous() if positions_per_window is not None else None
    P = int(ppw.shape[1]) if ppw is not None else len(positions)
    srcf = src.contiguous()
    out = torch.empty((B, P, D if average else 2 * D), dtype=torch.float32 if average else src.dtype, device=src.device)
    arr = (C.c_int32 * max(P, 1))(*[int(p) for p in positions]) if positions is not None else None
    with torch.cuda.device(src.device):
        _check(lib.pcad_layer_rows(srcf.data_ptr(), out.data_ptr(), B, L, D, arr, P, _ptr(ppw),
                                   int(bool(assembled)), int(bool(average)), _ptr(status),
                                   _dt(srcf), _stream_ptr()), "pcad_layer_rows")
    return out


# ---- the masked-LM loss head and its backward (include/pcad.h pcad_loss_head, include/pcad_bwd.h pcad_loss_head_bwd) ----
LOSS_SEG = 64            # csrc/kernels.hpp LOSS_SEG: positions per block of the loss head and of its backward (one row of partials each)


def _head_rows(h, res, B, L) -> int:
    """the checks both heads make on their 2B-strand rows h, res [2 B L, D] -> D"""
    D = h.shape[-1]
    if h.numel() != 2 * B * L * D or res.numel() != 2 * B * L * D:
        raise ValueError(f"h and res must be [2 B L, D] = [{2 * B * L}, {D}], got {tuple(h.shape)} and {tuple(res.shape)}")
    if res.dtype != torch.float32 and res.dtype != h.dtype:
        raise ValueError(f"res must be fp32 or h's dtype, got {res.dtype} for {h.dtype}")
    return D


def _head_batch(h, B, L):
    """B, L of a head's `*_fn` form: as given, else read from h [2B, L, D]"""
    if B is None or L is None:
        if h.dim() != 3:
            raise ValueError("h must be [2B, L, D], or [2B*L, D] with B= and L=")
        B, L = h.shape[0] // 2, h.shape[1]
    return B, L


class _WantedGrads:
    """The `want` of the two head backward wrappers.  spec: name -> (shape the kernel writes, dtype, shape handed back) of every gradient
    the kernel can form; the wanted ones get a `_guarded` output, the others are passed as NULL and come back as None."""

    def __init__(self, want, spec, dev, poison):
        if set(want) - set(spec) or not want:
            raise ValueError(f"want must name some of {', '.join(spec)}, got {tuple(want)}")
        self.spec = spec
        self.outs = {k: _guarded(sh, ty, dev, "row", poison) for k, (sh, ty, _) in spec.items() if k in want}

    def ptr(self, k):
        return self.outs[k][0].data_ptr() if k in self.outs else None

    def result(self, wrapper):
        """-> namespace(one field per name of the spec, guards_ok); wrapper.last_outputs: the names that were computed"""
        wrapper.last_outputs = tuple(k for k in self.spec if k in self.outs)
        fields = {k: self.outs[k][0].view(back) if k in self.outs else None for k, (_, _, back) in self.spec.items()}
        return SimpleNamespace(**fields, guards_ok=_guards_intact(self.outs.values()))


def _loss_head_operands(h, res, norm_weight, emb, complement, labels, loss_weights, B, L):
    if emb.shape[0] != 8:
        raise ValueError(f"emb must hold the 8 rows of the padded vocabulary, got {tuple(emb.shape)}")
    _head_rows(h, res, B, L)
    dev = h.device
    comp = torch.as_tensor(list(complement), dtype=torch.int32, device=dev) if not torch.is_tensor(complement) else complement.to(dev, torch.int32)
    return (h.contiguous(), res.contiguous(), norm_weight.float().contiguous(), emb.to(h.dtype).float().contiguous(), comp.contiguous(),
            labels.to(dev, torch.int32).contiguous(), loss_weights.to(dev, torch.float32).contiguous() if loss_weights is not None else None)


def loss_head(h, res, norm_weight, emb, complement, labels, loss_weights=None, ignore_index=-100, eps=1e-5, *, B: int, L: int,
              want_nll: bool = False, want_logits: bool = False):
    """norm_f + RC re-assembly + tied RCPS LM head + weighted cross entropy of the labelled positions (include/pcad.h pcad_loss_head).
    h [2B*L, D], res [2B*L, D] (fp32 or h.dtype), emb [8, D] (rounded to h.dtype here, as the tied lm_head weight is), labels [B, L]
    (ignored: == ignore_index or negative), loss_weights [B, L] or None.
    -> (sums fp32 [B, 4] = sum w nll, sum w, labelled, arg-max hits per window; nll fp32 [B, L] | None; logits fp32 [B, L, 8] | None)."""
    _require_gpu(h, "h")
    lib = load_library()
    D, dev = h.shape[-1], h.device
    hf, rf, w, e32, comp, lab, wt = _loss_head_operands(h, res, norm_weight, emb, complement, labels, loss_weights, B, L)
    sums = torch.empty((B, 4), dtype=torch.float32, device=dev)
    nll = torch.empty((B, L), dtype=torch.float32, device=dev) if want_nll else None
    lg = torch.empty((B, L, 8), dtype=torch.float32, device=dev) if want_logits else None
    nb = lib.pcad_loss_head_scratch_bytes(B, L)
    scratch, scratch_ptr = _scratch(nb, dev)
    with torch.cuda.device(dev):
        _check(lib.pcad_loss_head(hf.data_ptr(), rf.data_ptr(), w.data_ptr(), e32.data_ptr(), comp.data_ptr(), lab.data_ptr(), _ptr(wt),
                                  int(ignore_index), sums.data_ptr(), _ptr(nll), _ptr(lg), B, L, D, float(eps), None, None, _dt(hf),
                                  _DT[rf.dtype], 0, scratch_ptr, nb, _stream_ptr()), "pcad_loss_head")
    return sums, nll, lg


def loss_head_bwd(h, res, norm_weight, emb, complement, labels, loss_weights=None, ignore_index=-100, eps=1e-5, *, B: int, L: int,
                  dsum, dnll=None, want=("dh", "dres", "dnorm_weight", "demb"), poison=False):
    """pcad_loss_head_bwd on loss_head's operands: dsum fp32 [B] (the gradient of sums[:, 0]) and dnll fp32 [B, L] or None (the
    gradient of nll).  want: the gradients to compute; the others are passed as NULL and come back as None.
    -> namespace(dh like h; dres like res; dnorm_weight fp32 (D); demb fp32 (8, D) - the gradient of the dtype-rounded fp32 table;
    guards_ok).  Rows of dh / dres at unlabelled positions are zeros.  poison (tests): as selective_scan_bwd."""
    _require_gpu(h, "h")
    lib = load_bwd_library()
    D, dev, rows = h.shape[-1], h.device, 2 * B * L
    hf, rf, w, e32, comp, lab, wt = _loss_head_operands(h, res, norm_weight, emb, complement, labels, loss_weights, B, L)
    g = _WantedGrads(want, {"dh": ((rows, D), hf.dtype, h.shape), "dres": ((rows, D), rf.dtype, res.shape),
                            "dnorm_weight": ((D,), torch.float32, (D,)), "demb": ((8, D), torch.float32, (8, D))}, dev, poison)
    gs = dsum.to(dev, torch.float32).contiguous()
    gn = dnll.to(dev, torch.float32).contiguous() if dnll is not None else None
    if gs.numel() != B or (gn is not None and gn.numel() != B * L):
        raise ValueError("dsum must be [B] and dnll [B, L]")
    nb = lib.pcad_loss_head_bwd_scratch_bytes(B, L, D)
    scratch, scratch_ptr = _scratch(nb, dev, poison)
    with torch.cuda.device(dev):
        _check(lib.pcad_loss_head_bwd(hf.data_ptr(), rf.data_ptr(), w.data_ptr(), e32.data_ptr(), comp.data_ptr(), lab.data_ptr(), _ptr(wt),
                                      int(ignore_index), gs.data_ptr(), _ptr(gn), g.ptr("dh"), g.ptr("dres"), g.ptr("dnorm_weight"), g.ptr("demb"),
                                      scratch_ptr, nb, B, L, D, float(eps), _dt(hf), _DT[rf.dtype], _stream_ptr()), "pcad_loss_head_bwd")
    return g.result(loss_head_bwd)


loss_head_bwd.last_outputs = ()      # the output set of the latest call (tests: a gradient nobody needs is not computed)


class _MlmLossHeadFn(torch.autograd.Function):
    """loss_head with a backward: pcad_loss_head_bwd (include/pcad_bwd.h, libpcad_bwd.so).  norm_weight and emb arrive in fp32 (emb
    already rounded to the model dtype; the casts are torch ops outside).  Only the inputs are saved; the kernel recomputes the
    logits.  Outputs: sums [B, 4] and nll [B, L]; only sums[:, 0] and nll are differentiable."""

    @staticmethod
    def forward(ctx, h, res, norm_weight, emb, complement, labels, loss_weights, ignore_index, eps, B, L):
        ctx.save_for_backward(h, res, norm_weight, emb, complement, labels, loss_weights)
        ctx.args = (int(ignore_index), float(eps), int(B), int(L))
        ctx.set_materialize_grads(False)
        sums, nll, _ = loss_head(h, res, norm_weight, emb, complement, labels, loss_weights, ignore_index, eps, B=B, L=L, want_nll=True)
        loss_sum, rest = sums[:, 0].contiguous(), sums[:, 1:].contiguous()
        ctx.mark_non_differentiable(rest)
        return loss_sum, rest, nll

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dsum, _drest, dnll):
        h, res, norm_weight, emb, complement, labels, loss_weights = ctx.saved_tensors
        ignore_index, eps, B, L = ctx.args
        need = ctx.needs_input_grad
        want = tuple(k for k, n in zip(("dh", "dres", "dnorm_weight", "demb"), need[:4]) if n)
        if dsum is None and dnll is None or not want:
            return (None,) * 11
        if dsum is None:
            dsum = torch.zeros(B, dtype=torch.float32, device=h.device)
        g = loss_head_bwd(h, res, norm_weight, emb, complement, labels, loss_weights, ignore_index, eps, B=B, L=L, dsum=dsum, dnll=dnll, want=want)
        return (g.dh, g.dres, g.dnorm_weight, g.demb) + (None,) * 7


def mlm_loss_head_fn(h, res, norm_weight, emb, complement, labels, loss_weights=None, ignore_index=-100, eps=1e-5, *, B: Optional[int] = None,
                     L: Optional[int] = None, return_nll: bool = False):
    """The end of CaduceusForMaskedLM's forward with labels - norm_f, RC re-assembly, the tied RCPS LM head and the weighted cross
    entropy - on the 2B-strand rows h, res [2B, L, D] (or [2B*L, D] with B=, L=).  -> sums fp32 [B, 4] (sum w nll, sum w, labelled,
    arg-max hits per window), and with return_nll the per-token nll fp32 [B, L] (0 at ignored positions).
    With grad mode on and one of h, res, norm_weight, emb requiring grad the call is differentiable (pcad_loss_head_bwd): each
    gradient comes back in its input's shape and dtype, gradients nobody needs are not computed, and only sums[:, 0] and nll carry a
    graph.  Otherwise it is the plain forward call."""
    _require_gpu(h, "h")
    B, L = _head_batch(h, B, L)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (h, res, norm_weight, emb)):
        comp = torch.as_tensor(list(complement), dtype=torch.int32, device=h.device) if not torch.is_tensor(complement) else complement
        # the casts stay torch ops outside the Function, so that autograd returns each gradient in its input's dtype
        loss_sum, rest, nll = _MlmLossHeadFn.apply(h, res, norm_weight.float(), emb.to(h.dtype).float(), comp, labels, loss_weights,
                                                   int(ignore_index), float(eps), B, L)
        sums = torch.cat([loss_sum.unsqueeze(1), rest], dim=1)
        return (sums, nll) if return_nll else sums
    sums, nll, _ = loss_head(h, res, norm_weight, emb, complement, labels, loss_weights, ignore_index, eps, B=B, L=L, want_nll=return_nll)
    return (sums, nll) if return_nll else sums


# ---- the pooled classification head and its backward (include/pcad.h pcad_pooled_head, include/pcad_bwd.h pcad_pooled_head_bwd) ----
POOL_BWD_SEG = 64        # csrc/kernels.hpp POOL_BWD_SEG: rows per block of the pooled head's backward (= the forward's segment)
TRAINABLE_POOLING = ("mean", "first", "last")       # max pooling has a forward only (include/pcad_bwd.h)


def _pooled_head_operands(h, res, norm_weight, score_w, pooling, B, L):
    if pooling not in POOLING:
        raise ValueError(f"pooling must be one of {sorted(POOLING)}, got {pooling!r}")
    D = _head_rows(h, res, B, L)
    if score_w.dim() != 2 or score_w.shape[1] != D or not 1 <= score_w.shape[0] <= MAX_LABELS:
        raise ValueError(f"score_w must be [1..{MAX_LABELS}, {D}], got {tuple(score_w.shape)}")
    # score_w is rounded to the model dtype here, as the score Linear's weight is stored in it
    return h.contiguous(), res.contiguous(), norm_weight.float().contiguous(), score_w.to(h.dtype).float().contiguous(), POOLING[pooling]


def pooled_head(h, res, norm_weight, score_w, pooling="mean", eps=1e-5, *, B: int, L: int, want_pooled: bool = False):
    """norm_f + per-strand pooling + score + (fwd + rc) / 2 (include/pcad.h pcad_pooled_head).  h [2B*L, D], res [2B*L, D] (fp32 or
    h.dtype), score_w [NL, D] (rounded to h.dtype here).  -> logits fp32 [B, NL], or with want_pooled (logits, pooled fp32 [B, 2, D])."""
    _require_gpu(h, "h")
    lib = load_library()
    D, dev = h.shape[-1], h.device
    hf, rf, w, W, pid = _pooled_head_operands(h, res, norm_weight, score_w, pooling, B, L)
    NL = W.shape[0]
    lg = torch.empty((B, NL), dtype=torch.float32, device=dev)
    pooled = torch.empty((B, 2, D), dtype=torch.float32, device=dev) if want_pooled else None
    nb = lib.pcad_pooled_head_scratch_bytes(B, L, D, pid)
    scratch, scratch_ptr = _scratch(nb, dev)
    with torch.cuda.device(dev):
        _check(lib.pcad_pooled_head(hf.data_ptr(), rf.data_ptr(), w.data_ptr(), W.data_ptr(), NL, _ptr(pooled), lg.data_ptr(), B, L, D,
                                    float(eps), pid, None, None, _dt(hf), _DT[rf.dtype], 0, scratch_ptr, nb, _stream_ptr()), "pcad_pooled_head")
    return (lg, pooled) if want_pooled else lg


def pooled_head_bwd(h, res, norm_weight, score_w, pooled, dlogits, pooling="mean", eps=1e-5, *, B: int, L: int,
                    want=("dh", "dres", "dnorm_weight", "dscore_w"), poison=False):
    """pcad_pooled_head_bwd on pooled_head's operands: pooled fp32 [B, 2, D] (the forward's) and dlogits fp32 [B, NL].  want: the
    gradients to compute; the others are passed as NULL and come back as None.
    -> namespace(dh like h; dres like res; dnorm_weight fp32 (D); dscore_w fp32 (NL, D) - the gradient of the dtype-rounded fp32 weight;
    guards_ok).  first / last: the rows the pooling did not read are zeros.  poison (tests): as selective_scan_bwd."""
    _require_gpu(h, "h")
    lib = load_bwd_library()
    D, dev, rows = h.shape[-1], h.device, 2 * B * L
    hf, rf, w, W, pid = _pooled_head_operands(h, res, norm_weight, score_w, pooling, B, L)
    NL = W.shape[0]
    g = _WantedGrads(want, {"dh": ((rows, D), hf.dtype, h.shape), "dres": ((rows, D), rf.dtype, res.shape),
                            "dnorm_weight": ((D,), torch.float32, (D,)), "dscore_w": ((NL, D), torch.float32, (NL, D))}, dev, poison)
    pl = pooled.to(dev, torch.float32).contiguous()
    gl = dlogits.to(dev, torch.float32).contiguous()
    if pl.numel() != B * 2 * D or gl.numel() != B * NL:
        raise ValueError(f"pooled must be [B, 2, D] and dlogits [B, NL] = [{B}, {NL}], got {tuple(pooled.shape)} and {tuple(dlogits.shape)}")
    nb = lib.pcad_pooled_head_bwd_scratch_bytes(B, L, D, pid)
    scratch, scratch_ptr = _scratch(nb, dev, poison)
    with torch.cuda.device(dev):
        _check(lib.pcad_pooled_head_bwd(hf.data_ptr(), rf.data_ptr(), w.data_ptr(), W.data_ptr(), pl.data_ptr(), gl.data_ptr(), g.ptr("dh"),
                                        g.ptr("dres"), g.ptr("dnorm_weight"), g.ptr("dscore_w"), scratch_ptr, nb, B, L, D, NL, float(eps), pid,
                                        _dt(hf), _DT[rf.dtype], _stream_ptr()), "pcad_pooled_head_bwd")
    return g.result(pooled_head_bwd)


pooled_head_bwd.last_outputs = ()    # the output set of the latest call (tests: a gradient nobody needs is not computed)


class _PooledHeadFn(torch.autograd.Function):
    """pooled_head with a backward: pcad_pooled_head_bwd (include/pcad_bwd.h, libpcad_bwd.so).  norm_weight and score_w arrive in fp32
    (the casts are torch ops outside).  score_w arrives UNROUNDED: forward and backward round it to the model dtype themselves (the
    wrappers' operand step), and dscore_w is returned as the kernel wrote it - the rounding is the identity in the derivative, where a
    torch cast pair outside would round the fp32 gradient to the model dtype on its way back.  Saved: the inputs and the forward's
    pooled_out."""

    @staticmethod
    def forward(ctx, h, res, norm_weight, score_w, pooling, eps, B, L):
        lg, pooled = pooled_head(h, res, norm_weight, score_w, pooling, eps, B=B, L=L, want_pooled=True)
        ctx.save_for_backward(h, res, norm_weight, score_w, pooled)
        ctx.args = (pooling, float(eps), int(B), int(L))
        return lg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits):
        h, res, norm_weight, score_w, pooled = ctx.saved_tensors
        pooling, eps, B, L = ctx.args
        want = tuple(k for k, n in zip(("dh", "dres", "dnorm_weight", "dscore_w"), ctx.needs_input_grad[:4]) if n)
        if not want:
            return (None,) * 8
        g = pooled_head_bwd(h, res, norm_weight, score_w, pooled, dlogits, pooling, eps, B=B, L=L, want=want)
        return (g.dh, g.dres, g.dnorm_weight, g.dscore_w) + (None,) * 4


def pooled_head_fn(h, res, norm_weight, score_w, pooling="mean", eps=1e-5, B: Optional[int] = None, L: Optional[int] = None):
    """The end of CaduceusForSequenceClassification's forward - norm_f, the per-strand pooling, the score head and the strand average -
    on the 2B-strand rows h, res [2B, L, D] (or [2B*L, D] with B=, L=).  -> logits fp32 [B, NL].
    With grad mode on and one of h, res, norm_weight, score_w requiring grad the call is differentiable (pcad_pooled_head_bwd): each
    gradient comes back in its input's shape and dtype (an fp32 score_w's is the kernel's fp32 dscore_w, straight through the rounding
    of score_w to the model dtype), gradients nobody
    needs are not computed, and max pooling is refused.  Otherwise it is the plain forward call."""
    _require_gpu(h, "h")
    B, L = _head_batch(h, B, L)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (h, res, norm_weight, score_w)):
        if pooling not in TRAINABLE_POOLING:
            raise NotImplementedError(f"pooling {pooling!r} has no backward (include/pcad_bwd.h): trainable poolings are {TRAINABLE_POOLING}")
        # the casts to fp32 stay torch ops outside the Function, so that autograd returns each gradient in its input's dtype; the rounding
        # of score_w to the model dtype happens inside it, so that an fp32 score_w receives the kernel's fp32 dscore_w bit for bit
        return _PooledHeadFn.apply(h, res, norm_weight.float(), score_w.float(), pooling, float(eps), B, L)
    return pooled_head(h, res, norm_weight, score_w, pooling, eps, B=B, L=L)


# ---- the score head on cached pooled vectors (include/pcad_bwd.h pcad_pooled_logits / pcad_pooled_logits_bwd) ----
def _pooled_logits_operands(pooled, score_w, dtype):
    """pooled fp32 [B, 2, D] on the GPU and score_w [NL, D] -> (pooled, the weight rounded to the model dtype `dtype` as fp32, B, D, NL)"""
    _require_gpu(pooled, "pooled")
    if dtype not in _DT:
        raise ValueError(f"unsupported dtype {dtype}: the model dtype is bf16 or fp32")
    if pooled.dim() != 3 or pooled.shape[1] != 2 or pooled.dtype != torch.float32:
        raise ValueError(f"pooled must be fp32 [B, 2, D], got {pooled.dtype} {tuple(pooled.shape)}")
    D = pooled.shape[2]
    if score_w.dim() != 2 or score_w.shape[1] != D or not 1 <= score_w.shape[0] <= MAX_LABELS:
        raise ValueError(f"score_w must be [1..{MAX_LABELS}, {D}], got {tuple(score_w.shape)}")
    # score_w is rounded to the model dtype here, as pooled_head and Engine.forward_pooled round it
    W = score_w.detach().to(pooled.device).to(dtype).float().contiguous()
    return pooled.detach().contiguous(), W, pooled.shape[0], D, W.shape[0]


def pooled_logits(pooled, score_w, dtype):
    """pcad_pooled_logits: the logits of cached pooled vectors - pooled fp32 [B, 2, D] (pooled_head's / Engine.forward_pooled's
    want_pooled output), score_w [NL, D] (rounded to the model dtype `dtype` here) -> logits fp32 [B, NL], the bits the head that
    produced `pooled` writes for the same weight."""
    lib = load_bwd_library()
    pl, W, B, D, NL = _pooled_logits_operands(pooled, score_w, dtype)
    lg = torch.empty((B, NL), dtype=torch.float32, device=pl.device)
    with torch.cuda.device(pl.device):
        _check(lib.pcad_pooled_logits(_ptr(pl) or None, W.data_ptr(), _ptr(lg) or None, B, D, NL, _DT[dtype], _stream_ptr()), "pcad_pooled_logits")
    return lg


def pooled_logits_bwd(pooled, score_w, dlogits, want=("dscore_w",), poison=False):
    """pcad_pooled_logits_bwd: pooled fp32 [B, 2, D], score_w [NL, D] as the forward took it (already rounded: there is no dtype here),
    dlogits fp32 [B, NL].  want: some of dscore_w, dpooled; the other is passed as NULL and comes back as None.
    -> namespace(dscore_w fp32 (NL, D); dpooled fp32 (B, 2, D); guards_ok).  poison (tests): as selective_scan_bwd."""
    lib = load_bwd_library()
    pl, W, B, D, NL = _pooled_logits_operands(pooled, score_w, torch.float32)
    g = _WantedGrads(want, {"dscore_w": ((NL, D), torch.float32, (NL, D)), "dpooled": ((B, 2, D), torch.float32, (B, 2, D))}, pl.device, poison)
    gl = dlogits.detach().to(pl.device, torch.float32).contiguous()
    if gl.numel() != B * NL:
        raise ValueError(f"dlogits must be [B, NL] = [{B}, {NL}], got {tuple(dlogits.shape)}")
    with torch.cuda.device(pl.device):
        _check(lib.pcad_pooled_logits_bwd(_ptr(pl) or None, W.data_ptr(), _ptr(gl) or None, g.ptr("dscore_w"), g.ptr("dpooled") or None, B, D, NL,
                                          _stream_ptr()), "pcad_pooled_logits_bwd")
    return g.result(pooled_logits_bwd)


pooled_logits_bwd.last_outputs = ()    # the output set of the latest call


class _PooledLogitsFn(torch.autograd.Function):
    """pooled_logits with a backward: pcad_pooled_logits_bwd.  score_w arrives in fp32 and UNROUNDED, as in _PooledHeadFn: forward and
    backward round it to the model dtype themselves and dscore_w is returned as the kernel wrote it, straight through the rounding."""

    @staticmethod
    def forward(ctx, pooled, score_w, dtype):
        ctx.save_for_backward(pooled, score_w)
        ctx.dtype = dtype
        return pooled_logits(pooled, score_w, dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits):
        pooled, score_w = ctx.saved_tensors
        want = tuple(k for k, n in zip(("dpooled", "dscore_w"), ctx.needs_input_grad[:2]) if n)
        if not want:
            return None, None, None
        g = pooled_logits_bwd(pooled, score_w.to(ctx.dtype).float(), dlogits, want=want)
        return g.dpooled, g.dscore_w, None


def pooled_logits_fn(pooled, score_w, dtype):
    """The score head on cached pooled vectors: pooled fp32 [B, 2, D], score_w [NL, D], the model dtype -> logits fp32 [B, NL].  With
    grad mode on and pooled or score_w requiring grad the call is differentiable (pcad_pooled_logits_bwd): an fp32 score_w receives the
    kernel's fp32 dscore_w bit for bit, straight through its rounding to the model dtype; a gradient nobody needs is not computed.
    Otherwise it is the plain call."""
    if torch.is_grad_enabled() and (pooled.requires_grad or score_w.requires_grad):
        return _PooledLogitsFn.apply(pooled, score_w.float(), dtype)
    return pooled_logits(pooled, score_w, dtype)


def _lora_merged(W, A, B, scale, dtype):
    """(W + scale B A) formed in fp32 (in float64 where the factors are float64: the CPU checks) and cast once to `dtype`"""
    acc = torch.promote_types(torch.float32, A.dtype)
    return (W.to(acc) + float(scale) * (B.to(acc) @ A.to(acc))).to(dtype)


class _LoraLinearFn(torch.autograd.Function):
    """y = x W_eff^T with W_eff = round(W + scale B A) in x's dtype: the merged form (adapters.merge_lora's arithmetic).  The backward
    never forms dW [N, K]: dx = dy W_eff, dB = scale dy^T (x A^T), dA = scale (dy B)^T x - rank-r GEMMs of stock PyTorch.  The rounding
    of W_eff is the identity in the derivative; W itself gets no gradient."""

    @staticmethod
    def forward(ctx, x, W, A, B, scale):
        w_eff = _lora_merged(W, A, B, scale, x.dtype)
        ctx.save_for_backward(x, w_eff, A, B)
        ctx.scale = float(scale)
        return F.linear(x, w_eff)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w_eff, A, B = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = dA = dB = None
        if need[0]:
            dx = dy @ w_eff
        if need[2] or need[3]:
            x2, g2 = x.reshape(-1, x.shape[-1]).to(A.dtype), dy.reshape(-1, dy.shape[-1]).to(A.dtype)
            if need[3]:
                dB = (ctx.scale * (g2.t() @ (x2 @ A.t()))).to(B.dtype)
            if need[2]:
                dA = (ctx.scale * ((g2 @ B).t() @ x2)).to(A.dtype)
        return dx, None, dA, dB, None


def lora_linear_fn(x, W, A, B, scale):
    """F.linear(x, (W.float() + scale * B @ A).to(x.dtype)): a frozen linear W [N, K] with the LoRA factors A [r, K], B [N, r] merged into
    it - the arithmetic of adapters.merge_lora, and so of inference with lora_deltas="apply".  A and B are fp32 whatever x's dtype.
    Differentiable in x, A and B through `_LoraLinearFn` (W gets no gradient); tensors on any device."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, A, B)):
        return _LoraLinearFn.apply(x, W, A, B, float(scale))
    return F.linear(x, _lora_merged(W, A, B, scale, x.dtype))


# ---- LoRA dropout: the unmerged form around the masked rank-r kernels (include/pcad_bwd.h pcad_lora_down / pcad_lora_down_bwd) ----
LORA_RANKS = (4, 8, 16)             # include/pcad_bwd.h: the ranks the kernels are built for
LORA_MIN_K, LORA_MAX_K = 8, 8192    # ... and K, a multiple of 8 inside this range
LORA_MASK_GUARD = 0x5A              # the sentinel byte around a poisoned mask


def lora_dropout_threshold(p: float) -> int:
    """T = floor(p 65536 + 0.5) of a drop probability; ValueError outside [0, 65535] (p < 0, p too close to 1, not finite)"""
    p = float(p)
    T = int(p * 65536.0 + 0.5) if p == p and 0.0 <= p < 2.0 else -1
    if not 0 <= T <= 65535:
        raise ValueError(f"lora dropout p must be in [0, 1) with floor(p 65536 + 0.5) <= 65535, got {p}")
    return T


def lora_dropout_limits(K: int, r: int, p: float = 0.0):
    """ValueError naming what of (K, r, p) lies outside the kernels' limits"""
    if r not in LORA_RANKS:
        raise ValueError(f"lora dropout: r must be one of {LORA_RANKS}, got {r}")
    if K % 8 or not LORA_MIN_K <= K <= LORA_MAX_K:
        raise ValueError(f"lora dropout: K must be a multiple of 8 in [{LORA_MIN_K}, {LORA_MAX_K}], got {K}")
    lora_dropout_threshold(p)


def lora_down_bwd_slabs(M: int, K: int, r: int):
    """pcad_lora_down_bwd_slabs (host only): -> (slabs, rows_per_slab) of the backward's split of the M rows; a refused shape raises"""
    rows = C.c_int64(0)
    slabs = load_bwd_library().pcad_lora_down_bwd_slabs(int(M), int(K), int(r), C.byref(rows))
    if slabs < 0:
        _check(1, "pcad_lora_down_bwd_slabs")
    return int(slabs), int(rows.value)


def _u64(v: int) -> int:
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError(f"seed and stream are unsigned 64-bit values, got {v}")
    return v


def _lora_rows(t: torch.Tensor, what: str):
    """t [..., K] bf16 / fp32 as M rows of K elements `ld` apart, in place when its layout allows it (unit stride inside a row, the
    leading dimensions collapsing to one row stride that is a multiple of 8 and >= K, a 16-byte aligned start), else through
    .contiguous().  -> (the tensor that owns the rows, M, ld)"""
    _dt(t)
    K = t.shape[-1]
    M = t.numel() // K if K else 0
    lead = [(n, s) for n, s in zip(t.shape[:-1], t.stride()[:-1]) if n != 1]
    ok = t.dim() >= 2 and t.stride(-1) == 1 and all(a[1] == b[0] * b[1] for a, b in zip(lead, lead[1:]))
    ld = lead[-1][1] if lead else K
    if not ok or ld % 8 or ld < K or t.data_ptr() % 16:
        t, ld = t.contiguous(), K
    return t, M, ld


def lora_dropout_mask(M: int, K: int, p: float, seed: int, stream: int, poison: bool = False):
    """pcad_lora_dropout_mask: the keep mask of (p, seed, stream) as a bool [M, K] tensor on the current device.  poison (tests): the
    kernel writes into a row-strided frame (K + 8 bytes per row) inside a buffer of sentinel bytes - one row above and below, 4 columns
    left and right; lora_dropout_mask.guards_ok tells whether they are intact."""
    lib = load_bwd_library()
    if K % 8 or not LORA_MIN_K <= K <= LORA_MAX_K:
        raise ValueError(f"lora dropout: K must be a multiple of 8 in [{LORA_MIN_K}, {LORA_MAX_K}], got {K}")
    lora_dropout_threshold(p)
    dev = torch.device("cuda", torch.cuda.current_device())
    if poison:
        whole = torch.full((M + 2, K + 8), LORA_MASK_GUARD, dtype=torch.uint8, device=dev)
        run = whole[1:M + 1, 4:K + 4]
    else:
        whole, run = None, torch.empty((M, K), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.pcad_lora_dropout_mask(run.data_ptr(), M, K, run.stride(0) if M else K, float(p), _u64(seed), _u64(stream), _stream_ptr()),
               "pcad_lora_dropout_mask")
    lora_dropout_mask.guards_ok = None
    if poison:
        outside = torch.ones_like(whole, dtype=torch.bool)
        outside[1:M + 1, 4:K + 4] = False
        lora_dropout_mask.guards_ok = bool((whole[outside] == LORA_MASK_GUARD).all()) and bool((run <= 1).all())
    return run != 0


lora_dropout_mask.guards_ok = None


def lora_down(x, A, p, seed, stream, poison=False):
    """pcad_lora_down: t[m, j] = c sum_k keep(m, k) x[m, k] A[j, k] -> fp32 [M, r] over the M rows of x [..., K] (bf16 or fp32; a
    row-strided view is read in place when its strides meet the limits, else copied); A fp32 [r, K].  Limits violated: ValueError.
    poison (tests): t starts as NaN between sentinel rows; lora_down.guards_ok tells whether they are intact."""
    _require_gpu(x, "x")
    _require_gpu(A, "A")
    lib = load_bwd_library()
    if A.dtype != torch.float32 or A.dim() != 2 or A.shape[1] != x.shape[-1]:
        raise ValueError(f"A must be fp32 [r, K = {x.shape[-1]}], got {A.dtype} {tuple(A.shape)}")
    r, K = A.shape
    lora_dropout_limits(K, r, p)
    xr, M, ldx = _lora_rows(x, "x")
    Ac = A.detach().contiguous()
    t, whole = _guarded((M, r), torch.float32, x.device, poison=poison)
    with torch.cuda.device(x.device):
        _check(lib.pcad_lora_down(xr.data_ptr(), ldx, Ac.data_ptr(), t.data_ptr(), M, K, r, float(p), _u64(seed), _u64(stream), _dt(xr),
                                  _stream_ptr()), "pcad_lora_down")
    lora_down.guards_ok = _guards_intact([(t, whole)]) if poison else None
    return t


lora_down.guards_ok = None


def lora_down_bwd(x, A, u, dx, p, seed, stream, want=("dx", "dA"), poison=False):
    """pcad_lora_down_bwd: with u = dL/dt fp32 [M, r],
        dA[j, k] = c sum_m keep(m, k) u[m, j] x[m, k]                          -> fp32 [r, K], a new tensor
        dx[m, k] = round(dx[m, k] + c keep(m, k) sum_j u[m, j] A[j, k])        IN PLACE on dx [..., K] in x's dtype (the caller's dx0)
    want: which of the two are computed.  -> (dx or None, dA or None).  dx must have unit stride inside a row and meet the kernel's
    stride limits - it is written, so it is never copied.
    poison (tests): the scratch starts as 0xFF bytes, dA as NaN between sentinels, and dx is updated on a copy inside a frame of
    sentinels (one row above and below, 8 columns left and right) that is copied back; lora_down_bwd.guards_ok tells whether all
    sentinels are intact."""
    _require_gpu(x, "x")
    lib = load_bwd_library()
    want = tuple(want)
    if not want or any(w not in ("dx", "dA") for w in want):
        raise ValueError(f"want must name 'dx', 'dA' or both, got {want}")
    r, K = A.shape
    lora_dropout_limits(K, r, p)
    xr, M, ldx = _lora_rows(x, "x")
    dev = x.device
    if A.dtype != torch.float32 or u.dtype != torch.float32 or tuple(u.shape) != (M, r) or K != x.shape[-1]:
        raise ValueError(f"A must be fp32 [r, K], u fp32 [M, r] = [{M}, {r}]; got {A.dtype} {tuple(A.shape)}, {u.dtype} {tuple(u.shape)}")
    Ac, uc = A.detach().contiguous(), u.contiguous()
    run = dxr = whole_dx = None
    lddx = K
    if "dx" in want:
        if dx is None or dx.dtype != x.dtype or dx.shape != x.shape or dx.device != dev:
            raise ValueError(f"dx must be a {x.dtype} tensor of x's shape {tuple(x.shape)} on {dev}")
        dxr, _, lddx = _lora_rows(dx, "dx")
        if dxr.data_ptr() != dx.data_ptr():
            raise ValueError("dx is updated in place: it needs unit stride inside a row, one row stride that is a multiple of 8 and a 16-byte aligned start")
        run = dxr
        if poison:
            whole_dx = torch.full((M + 2, K + 16), GUARD, dtype=x.dtype, device=dev)
            run = whole_dx[1:M + 1, 8:K + 8]
            run.copy_(dx.reshape(M, K))
            lddx = K + 16
    dA, whole_dA = _guarded((r, K), torch.float32, dev, poison=poison) if "dA" in want else (None, None)
    nb = lib.pcad_lora_down_bwd_scratch_bytes(M, K, r) if dA is not None else 0
    scratch, scratch_ptr = _scratch(nb, dev, poison)
    with torch.cuda.device(dev):
        _check(lib.pcad_lora_down_bwd(xr.data_ptr(), ldx, Ac.data_ptr(), uc.data_ptr(), _ptr(run), lddx, _ptr(dA), scratch_ptr, nb, M, K, r,
                                      float(p), _u64(seed), _u64(stream), _dt(xr), _stream_ptr()), "pcad_lora_down_bwd")
    lora_down_bwd.guards_ok = None
    if poison:
        if run is not None:
            with torch.no_grad():
                dx.copy_(run.reshape(dx.shape))
        lora_down_bwd.guards_ok = _guards_intact([(dA, whole_dA)] + ([(run, whole_dx)] if run is not None else []))
    return (dx if "dx" in want else None), dA


lora_down_bwd.guards_ok = None


def _lora_dropout_forward(x, w, A, B, scale, p, seed, stream):
    """-> (y, t): y = F.linear(x, w) + (scale t B^T) in x's dtype, t = pcad_lora_down's fp32 [M, r]"""
    t = lora_down(x, A, p, seed, stream)
    y = F.linear(x, w)
    return y + (float(scale) * (t @ B.t())).to(x.dtype).view(y.shape), t


class _LoraDropoutLinearFn(torch.autograd.Function):
    """y = x W^T + scale (c (keep x) A^T) B^T: a frozen linear with an UNMERGED LoRA branch whose input is dropped out by the mask of
    (p, seed, stream) (include/pcad_bwd.h).  Saved: x, the cast W, A, B and the fp32 [M, r] down-projection t; the mask is regenerated
    in the backward from (seed, stream, p) on ctx - there is no mask tensor and no dropped copy of x.  W gets no gradient."""

    @staticmethod
    def forward(ctx, x, W, A, B, scale, p, seed, stream):
        w = W.to(x.dtype)
        y, t = _lora_dropout_forward(x, w, A, B, scale, p, seed, stream)
        ctx.save_for_backward(x, w, A, B, t)
        ctx.scale, ctx.mask = float(scale), (float(p), int(seed), int(stream))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w, A, B, t = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = dy.reshape(-1, dy.shape[-1])
        gf = g.float()
        dx = dA = dB = None
        if need[3]:
            dB = ctx.scale * (gf.t() @ t)
        want = tuple(n for n, k in (("dx", need[0]), ("dA", need[2])) if k)
        if want:
            u = ctx.scale * (gf @ B)
            dx0 = g.mm(w).view(x.shape) if need[0] else None
            dx, dA = lora_down_bwd(x, A, u, dx0, *ctx.mask, want=want)
        return dx, None, dA, dB, None, None, None, None


def lora_dropout_linear_fn(x, W, A, B, scale, p, seed, stream):
    """F.linear(x, W.to(x.dtype)) + (scale * F.linear(F.linear(dropout(x), A), B)).to(x.dtype) with the dropout mask of (p, seed, stream)
    (DESIGN.md §4u): the unmerged LoRA form - the only one in which a dropout on the branch alone has a place.  x [..., K] bf16 or fp32
    on the device, W [N, K] frozen, A [r, K] and B [N, r] fp32.  A torch.autograd.Function when x, A or B requires grad, else the plain
    forward.  A non-contiguous x is read in place when its strides meet the kernels' limits, else copied.  r outside {4, 8, 16}, K not a
    multiple of 8 in [8, 8192] or a p outside [0, 1): ValueError naming the limit - there is no torch fallback."""
    _require_gpu(x, "x")
    if A.dtype != torch.float32 or B.dtype != torch.float32 or A.dim() != 2 or B.dim() != 2 or B.shape[1] != A.shape[0]:
        raise ValueError(f"A [r, K] and B [N, r] must be fp32, got {A.dtype} {tuple(A.shape)} and {B.dtype} {tuple(B.shape)}")
    if tuple(W.shape) != (B.shape[0], A.shape[1]) or x.shape[-1] != A.shape[1]:
        raise ValueError(f"W must be [N, K] = [{B.shape[0]}, {A.shape[1]}] and x [..., K], got {tuple(W.shape)} and {tuple(x.shape)}")
    lora_dropout_limits(A.shape[1], A.shape[0], p)
    _u64(seed), _u64(stream)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, A, B)):
        return _LoraDropoutLinearFn.apply(x, W, A, B, float(scale), float(p), int(seed), int(stream))
    return _lora_dropout_forward(x, W.to(x.dtype), A, B, scale, p, seed, stream)[0]


# ---- the optimizer step (include/pcad_bwd.h pcad_optim_plan / pcad_adamw_step / pcad_zero_grads) and the gathering of
# ---- every gradient into one fp32 buffer for a collective (pcad_grads_flat_plan / pcad_grads_gather) ------------------
OPTIM_CHUNK = 4096       # include/pcad_bwd.h PCAD_OPTIM_CHUNK = csrc/kernels.hpp OPTIM_CHUNK: elements per chunk = per block
OPTIM_DECAY = 1          # include/pcad_bwd.h PCAD_OPTIM_DECAY: flags bit 0


def _optim_record_type():

    class Record(C.Structure):            # include/pcad_bwd.h pcad_optim_tensor
        _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("master", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                    ("n", C.c_int64), ("param_dtype", C.c_int32), ("grad_dtype", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]
    assert C.sizeof(Record) == 64
    return Record


def _record_table(records):
    """host records (param, grad, master, exp_avg, exp_avg_sq, n, param_dtype, grad_dtype, flags) -> a ctypes array of pcad_optim_tensor"""
    tab = (_optim_record_type() * max(1, len(records)))()
    for r, rec in zip(tab, records):
        r.param, r.grad, r.master, r.exp_avg, r.exp_avg_sq, r.n, r.param_dtype, r.grad_dtype, r.flags = rec
    return tab


def optim_plan(records):
    """pcad_optim_plan on host records (param, grad, master, exp_avg, exp_avg_sq, n, param_dtype, grad_dtype, flags): pointers as
    integers or None, nothing is dereferenced.  -> (the table as bytes, the chunk map as a list of (record, chunk) pairs)"""
    lib = load_bwd_library()
    tab = _record_table(records)
    chunks = C.c_int64(0)
    _check(lib.pcad_optim_plan(C.addressof(tab), len(records), None, 0, C.byref(chunks)), "pcad_optim_plan")
    cmap = (C.c_int32 * max(2, 2 * chunks.value))()
    _check(lib.pcad_optim_plan(C.addressof(tab), len(records), C.addressof(cmap), chunks.value, C.byref(chunks)), "pcad_optim_plan")
    return bytes(tab)[:64 * len(records)], [(cmap[2 * c], cmap[2 * c + 1]) for c in range(chunks.value)]


def grads_flat_plan(records):
    """pcad_grads_flat_plan on host records (as optim_plan takes them; needs no device): where each tensor's gradient lies in one fp32
    buffer, every slice padded to a multiple of 4 elements (16 bytes).  -> (offsets in elements, one per record; total elements)"""
    lib = load_bwd_library()
    tab = _record_table(records)
    offsets = (C.c_int64 * max(1, len(records)))()
    total = C.c_int64(0)
    _check(lib.pcad_grads_flat_plan(C.addressof(tab), len(records), C.addressof(offsets), C.byref(total)), "pcad_grads_flat_plan")
    return [int(offsets[i]) for i in range(len(records))], int(total.value)


def _check_flat(flat, total: int, dev):
    """the one gradient buffer of a data-parallel step: a contiguous fp32 vector of at least the flat plan's total elements on `dev`"""
    if flat.dtype != torch.float32 or flat.dim() != 1 or not flat.is_contiguous() or flat.numel() < total or flat.device != dev:
        raise ValueError(f"flat must be a contiguous fp32 vector of at least {total} elements on {dev}")


class OptimTable:
    """The parameter set of pcad_adamw_step / pcad_zero_grads in device memory: one record per tensor and the chunk map beside it.
    params[i] / grads[i]: contiguous bf16 or fp32 tensors of equal size; masters[i]: fp32 or None (an fp32 parameter is its own
    master); exp_avgs[i], exp_avg_sqs[i]: fp32; decay[i]: whether weight decay applies.  Every data pointer must be 16-byte aligned
    (the plan refuses the table otherwise).  The upload goes on the current stream from pinned memory, without synchronising.
    state (fp32-sized [4] int32 tensor, include/pcad_bwd.h pcad_optim_state) is the caller's when given, so that it outlives the table."""

    def __init__(self, params, grads, masters, exp_avgs, exp_avg_sqs, decay, state=None):
        import numpy as np
        lists = (params, grads, masters, exp_avgs, exp_avg_sqs, decay)
        if len({len(x) for x in lists}) != 1:
            raise ValueError("params, grads, masters, exp_avgs, exp_avg_sqs and decay must have one entry per tensor")
        self.params, self.grads, self.masters = list(params), list(grads), list(masters)
        self.exp_avgs, self.exp_avg_sqs, self.decay = list(exp_avgs), list(exp_avg_sqs), [bool(d) for d in decay]
        if not self.params:
            raise ValueError("an empty parameter set")
        dev = self.params[0].device
        records = []
        for i, (p, g, ms, m, v, d) in enumerate(zip(*lists)):
            for t, name, want in ((p, "param", None), (g, "grad", None), (ms, "master", torch.float32), (m, "exp_avg", torch.float32),
                                  (v, "exp_avg_sq", torch.float32)):
                if t is None and name == "master":
                    continue
                _require_gpu(t, f"{name}[{i}]")
                if t.device != dev or not t.is_contiguous() or t.numel() != p.numel() or (want is not None and t.dtype != want):
                    raise ValueError(f"{name}[{i}] must be a contiguous {want or 'bf16 / fp32'} tensor of param[{i}]'s size on {dev}")
            ptrs = [_ptr(t) if p.numel() else None for t in (p, g, ms, m, v)]            # an empty tensor has no address to hand over
            records.append((*ptrs, p.numel(), _dt(p), _dt(g), OPTIM_DECAY if d else 0))
        self.pointers = tuple(r[:5] for r in records)
        self.records = records
        self._flat_plan, self._flat_offsets = None, None
        tab, cmap = optim_plan(records)
        self.count, self.chunks = len(records), len(cmap)
        host = torch.from_numpy(np.frombuffer(tab, dtype=np.uint8).copy()).pin_memory()
        hmap = torch.tensor(cmap if cmap else [(0, 0)], dtype=torch.int32).pin_memory()
        with torch.cuda.device(dev):
            self._host = (host, hmap)                                 # alive until the copies have run
            self.table = host.to(dev, non_blocking=True)
            self.chunk_map = hmap.to(dev, non_blocking=True)
            self.state = state if state is not None else torch.zeros(4, dtype=torch.int32, device=dev)
            self.scratch_bytes = load_bwd_library().pcad_adamw_step_scratch_bytes(self.chunks)
            self.scratch, self.scratch_ptr = _scratch(self.scratch_bytes, dev)
        self.device = dev

    def flat_plan(self):
        """-> (offsets, total) of grads_flat_plan for this table: the layout of its gradients in one fp32 buffer"""
        if self._flat_plan is None:
            self._flat_plan = grads_flat_plan(self.records)
        return self._flat_plan

    def flat_offsets(self) -> torch.Tensor:
        """the offsets of flat_plan() as a device int64 tensor, uploaded once on the current stream from pinned memory"""
        if self._flat_offsets is None:
            host = torch.tensor(self.flat_plan()[0] or [0], dtype=torch.int64).pin_memory()
            with torch.cuda.device(self.device):
                self._flat_offsets = (host.to(self.device, non_blocking=True), host)
        return self._flat_offsets[0]

    def on_flat(self, flat: torch.Tensor) -> "OptimTable":
        """The second table of a data-parallel step: the same parameters, masters, moments, decay flags and state - no
        second set of anything - with the gradient of tensor i the fp32 slice flat[offsets[i] : offsets[i] + n_i] that grads_gather fills.
        flat: a contiguous fp32 tensor of at least flat_plan()'s total elements on this device, 16-byte aligned."""
        offsets, total = self.flat_plan()
        _check_flat(flat, total, self.device)
        slices = [flat[o:o + p.numel()].view(p.shape) for o, p in zip(offsets, self.params)]
        return OptimTable(self.params, slices, self.masters, self.exp_avgs, self.exp_avg_sqs, self.decay, state=self.state)

    def read_state(self):
        """-> dict(norm, coef, finite, skipped) of the last step.  Synchronises."""
        raw = self.state.cpu()
        f = raw.view(torch.float32)
        return {"norm": float(f[0]), "coef": float(f[1]), "finite": int(raw[2]), "skipped": int(raw[3])}


def adamw_step(table: OptimTable, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, max_norm=0.0, grad_scale=1.0,
               poison=False):
    """pcad_adamw_step: one AdamW step with global-norm clipping over the table's tensors, in place (torch.optim.AdamW's arithmetic in
    fp32 after clip_grad_norm_(max_norm) of grad_scale * grad; max_norm <= 0: no clipping; `step` is the 1-based step number of the
    bias corrections).  Non-finite gradients: nothing changes and the state's `skipped` goes up.  No host synchronisation.
    poison (tests): the step runs on copies of every output - param, master, exp_avg, exp_avg_sq - that sit between OPTIM_GUARD sentinel
    elements, with a scratch of 0xFF bytes, and the results are copied back; -> whether all sentinels are intact (else None)."""
    lib = load_bwd_library()
    bc1, bc2 = 1.0 - float(beta1) ** int(step), 1.0 - float(beta2) ** int(step)
    run, back = table, []
    if poison:
        cols = [_guarded_copies(src, back) for src in (table.params, table.masters, table.exp_avgs, table.exp_avg_sqs)]
        run = OptimTable(cols[0], table.grads, cols[1], cols[2], cols[3], table.decay, state=table.state)
        run.scratch, run.scratch_ptr = _scratch(run.scratch_bytes, table.device, poison=True)
    with torch.cuda.device(table.device):
        _check(lib.pcad_adamw_step(run.table.data_ptr(), run.chunk_map.data_ptr(), run.count, run.chunks, run.state.data_ptr(),
                                   run.scratch_ptr, run.scratch_bytes, float(lr), float(beta1), float(beta2), float(eps),
                                   float(weight_decay), bc1, bc2, float(max_norm), float(grad_scale), _stream_ptr()), "pcad_adamw_step")
    return _copy_back(back) if poison else None


def zero_grads(table: OptimTable, poison=False):
    """pcad_zero_grads: every gradient of the table set to zero in one launch, storage kept.  poison (tests): as adamw_step, on guarded
    NaN-filled copies of the gradients."""
    lib = load_bwd_library()
    run, back = table, []
    if poison:
        grads = _guarded_copies(table.grads, back, blank=True)
        run = OptimTable(table.params, grads, table.masters, table.exp_avgs, table.exp_avg_sqs, table.decay, state=table.state)
    with torch.cuda.device(table.device):
        _check(lib.pcad_zero_grads(run.table.data_ptr(), run.chunk_map.data_ptr(), run.count, run.chunks, _stream_ptr()), "pcad_zero_grads")
    return _copy_back(back) if poison else None


def grads_gather(table: OptimTable, flat: torch.Tensor, offsets: torch.Tensor, poison=False):
    """pcad_grads_gather: every gradient of the table, widened to fp32 (exact), into its slice of `flat` in one launch over the table's own
    chunk map: flat[offsets[i] + k] = float(grad_i[k]).  offsets: table.flat_offsets() (device int64, table.flat_plan()'s); flat: a
    contiguous fp32 vector of at least the plan's total elements, 16-byte aligned.  The padding of a slice (up to 3 elements) and whatever
    lies beyond the total are not written, the gradients are not modified.  No host synchronisation.
    poison (tests): the launch runs on a copy of flat between OPTIM_GUARD sentinel elements and the result is copied back; -> whether all
    sentinels are intact (else None)."""
    lib = load_bwd_library()
    _require_gpu(flat, "flat")
    _require_gpu(offsets, "offsets")
    _check_flat(flat, table.flat_plan()[1], table.device)
    if offsets.dtype != torch.int64 or not offsets.is_contiguous() or offsets.numel() < table.count or offsets.device != table.device:
        raise ValueError(f"offsets must be a contiguous int64 tensor of {table.count} elements on {table.device}")
    run, back = flat, []
    if poison:
        run, = _guarded_copies([flat], back)
    with torch.cuda.device(table.device):
        _check(lib.pcad_grads_gather(table.table.data_ptr(), table.chunk_map.data_ptr(), table.count, table.chunks, offsets.data_ptr(),
                                     run.data_ptr(), run.numel(), _stream_ptr()), "pcad_grads_gather")
    return _copy_back(back) if poison else None


# ---- fp32 main gradients: the weight gradient of a linear layer, accumulated in place (include/pcad_bwd.h pcad_linear_wgrad) ----
WGRAD_MIN, WGRAD_MAX = 8, 8192      # include/pcad_bwd.h: N and K are multiples of 8 inside [8, 8192]
WGRAD_GUARD = GUARD                 # the sentinel around a poisoned output (rows above and below, 4 columns left and right)

_log = logging.getLogger(__name__)


def linear_wgrad_slabs(M: int, N: int, K: int):
    """pcad_linear_wgrad_slabs (host only): -> (slabs, rows_per_slab) of the split of the M rows; a refused shape raises"""
    rows = C.c_int64(0)
    slabs = load_bwd_library().pcad_linear_wgrad_slabs(int(M), int(N), int(K), C.byref(rows))
    if slabs < 0:
        _check(1, "pcad_linear_wgrad_slabs")
    return int(slabs), int(rows.value)


def wgrad_kernel_takes(N: int, K: int) -> bool:
    """whether [N, K] lies inside pcad_linear_wgrad's limits"""
    return N % 8 == 0 and K % 8 == 0 and WGRAD_MIN <= N <= WGRAD_MAX and WGRAD_MIN <= K <= WGRAD_MAX


def _wgrad_rows(t: torch.Tensor, what: str):
    """t [..., C] bf16 as M rows of C elements `ld` apart, in place when its layout allows it (unit stride inside a row, the leading
    dimensions collapsing to one row stride that is a multiple of 8 and >= C, a 16-byte aligned start), else through .contiguous().
    -> (the tensor that owns the rows, M, ld)"""
    if t.dtype != torch.bfloat16:
        raise ValueError(f"{what} must be bf16 (an fp32 model's gradients are fp32 already), got {t.dtype}")
    C = t.shape[-1]
    M = t.numel() // C if C else 0
    lead = [(n, s) for n, s in zip(t.shape[:-1], t.stride()[:-1]) if n != 1]
    ok = t.dim() >= 2 and t.stride(-1) == 1 and all(a[1] == b[0] * b[1] for a, b in zip(lead, lead[1:]))
    ld = lead[-1][1] if lead else C
    if not ok or ld % 8 or ld < C or t.data_ptr() % 16:
        t, ld = t.contiguous(), C
    return t, M, ld


def linear_wgrad(dy, x, out=None, accumulate=False, poison=False):
    """pcad_linear_wgrad: out[n, k] = (accumulate ? out[n, k] : 0) + sum_m dy[m, n] x[m, k] in fp32, the products exact and the sum in a
    fixed order.  dy [..., N] and x [..., K] bf16 over the same leading dimensions (M rows); a row-strided view such as x_dbl[..., :R] is
    read in place when its strides meet the kernel's limits, else copied.  out: fp32 [N, K] with unit stride inside a row (a row stride
    that is a multiple of 4, a 16-byte aligned start), written in place; None: a new tensor (accumulate then adds to zeros).
    -> out.  poison (tests): the scratch starts as 0xFF bytes and the call runs on a copy of out inside a larger buffer of sentinels -
    one row above and below, 4 columns left and right - that is copied back; linear_wgrad.guards_ok tells whether they are intact."""
    _require_gpu(dy, "dy")
    _require_gpu(x, "x")
    lib = load_bwd_library()
    N, K, dev = dy.shape[-1], x.shape[-1], dy.device
    if dy.shape[:-1] != x.shape[:-1]:
        raise ValueError(f"dy and x must share their leading dimensions, got {tuple(dy.shape)} and {tuple(x.shape)}")
    dyr, M, lddy = _wgrad_rows(dy, "dy")
    xr, _, ldx = _wgrad_rows(x, "x")
    if out is None:
        out = torch.zeros((N, K), dtype=torch.float32, device=dev) if accumulate else torch.empty((N, K), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != (N, K) or out.device != dev or (K > 1 and out.stride(1) != 1):
        raise ValueError(f"out must be an fp32 [{N}, {K}] tensor on {dev} with unit stride inside a row")
    run, whole = out, None
    if poison:
        whole = torch.full((N + 2, K + 8), WGRAD_GUARD, dtype=torch.float32, device=dev)
        run = whole[1:N + 1, 4:K + 4]
        run.copy_(out if accumulate else torch.full_like(out, float("nan")))
    nb = lib.pcad_linear_wgrad_scratch_bytes(M, N, K)
    scratch, scratch_ptr = _scratch(nb, dev, poison)
    with torch.cuda.device(dev):
        _check(lib.pcad_linear_wgrad(dyr.data_ptr(), lddy, xr.data_ptr(), ldx, run.data_ptr(), run.stride(0), M, N, K, int(bool(accumulate)),
                                     scratch_ptr, nb, _stream_ptr()), "pcad_linear_wgrad")
    linear_wgrad.guards_ok = None
    if poison:
        with torch.no_grad():
            out.copy_(run)
        linear_wgrad.guards_ok = _guards_intact([(run, whole)])
    return out


linear_wgrad.guards_ok = None       # whether the sentinels of the latest poisoned call are intact (None: it was not poisoned)
_wgrad_fallback_logged = set()


def _main_grad_add(main_grad, dy, x):
    """main_grad += dy^T x over the rows of dy [..., N] / x [..., K]: pcad_linear_wgrad(accumulate=1) for bf16 device operands and an fp32
    main_grad inside the kernel's limits; otherwise the same product by torch.addmm on copies in main_grad's dtype (fp32 in training)"""
    N, K = dy.shape[-1], x.shape[-1]
    if dy.is_cuda and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and main_grad.dtype == torch.float32 and wgrad_kernel_takes(N, K):
        linear_wgrad(dy, x, out=main_grad, accumulate=True)
        return
    key = (N, K, dy.dtype, str(dy.device.type))
    if key not in _wgrad_fallback_logged:
        _wgrad_fallback_logged.add(key)
        _log.debug("linear_fn: [%d, %d] %s on %s is outside pcad_linear_wgrad's limits; its weight gradient is formed by torch.addmm in %s",
                   N, K, dy.dtype, dy.device.type, main_grad.dtype)
    main_grad.addmm_(dy.reshape(-1, N).to(main_grad.dtype).t(), x.reshape(-1, K).to(main_grad.dtype))


class _LinearMainGradFn(torch.autograd.Function):
    """F.linear(x, weight) whose weight gradient goes to weight.main_grad instead of weight.grad: the forward is the stock call,
    dx = dy W is the stock product, dy^T x is ADDED to main_grad (fp32, never rounded to the weight's dtype) and the weight receives
    None.  A weight used twice (tied in_proj / out_proj) simply accumulates twice.  Saved: x and weight, through save_for_backward only
    (gradient checkpointing's hooks see both); main_grad is no activation and rides on ctx."""

    @staticmethod
    def forward(ctx, x, weight, main_grad):
        ctx.save_for_backward(x, weight)
        ctx.main_grad = main_grad
        return F.linear(x, weight.to(x.dtype))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        # stock F.linear flattens to 2-d, so its backward is this mm on the flattened dy: the same call, the same bits
        dx = dy.reshape(-1, dy.shape[-1]).mm(weight.to(dy.dtype)).view(x.shape) if ctx.needs_input_grad[0] else None
        if ctx.needs_input_grad[1]:
            _main_grad_add(ctx.main_grad, dy, x)
        return dx, None, None


def linear_fn(x, weight):
    """F.linear(x, weight.to(x.dtype)) for the trainable masked LM's projections.  A weight without a `main_grad` attribute - the
    default - IS that call: the same autograd node, the gradient in weight.grad.  A weight whose `main_grad` is a tensor of its shape
    (fp32; optim.AdamW(fp32_grad_accumulation=True) sets it), with grad mode on and the weight requiring grad: the same forward, and
    the backward adds dy^T x to main_grad - by pcad_linear_wgrad for bf16 operands inside its limits, else by torch.addmm - and leaves
    weight.grad alone."""
    mg = getattr(weight, "main_grad", None)
    if mg is None or not torch.is_grad_enabled() or not weight.requires_grad:
        return F.linear(x, weight.to(x.dtype))
    if not isinstance(mg, torch.Tensor) or mg.shape != weight.shape or mg.device != weight.device:
        raise ValueError(f"main_grad must be a tensor of the weight's shape {tuple(weight.shape)} on {weight.device}")
    return _LinearMainGradFn.apply(x, weight, mg)
