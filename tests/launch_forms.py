"""The engine's small-launch policy restated in Python (test helper; no tests here).

A pcad_forward call runs one of four layer walks, picked from the windows of the CALL (not of the chunk):
  segmented scan      csrc/kernels.hpp::scan_segments      few scan waves, L >= 256
  pair walk           csrc/kernels.hpp::scan_pair_wanted   both directions in one launch, half a strand each, twice
  conv + x_proj split csrc/convx.hip::convx_ksplit         ks blocks per row tile + a reduce kernel
  plain walk          everything else
Each form but the plain walk carves a scratch buffer of its own in the workspace (csrc/api.hip::carve_workspace), and only when it
runs, so `pcad_workspace_bytes` of a call minus that of the same call under "scan_segments" 0 (which switches all three off) names
the forms exactly.  `engaged_forms` checks that difference against the restatement below: a test that names a form asserts it ran,
and a bound moved in the C++ without moving it here fails tests/test_launch_forms.py."""
import ctypes as C

import torch

from plantcaduceus_amd import engine

# csrc/kernels.hpp / csrc/convx.hip constants
SEG_WAVES_SHORT = 512          # segmented scan: at most this many waves per direction for 256 <= L < 2048
SEG_WAVES_LONG = 768           # ... and for L >= 2048
SEG_TARGET_WAVES = 2304        # segments: enough for ~2 300 waves
PAIR_MAX_WAVES = 3584          # pair walk: at most this many waves per direction
CX_ROWS = 128                  # conv + x_proj: timesteps per row tile
CX_ROWB = 128                  # conv + x_proj: bytes of K per K-tile row
CX_SPLIT_TILES = 64            # conv + x_proj K-split: at most this many row tiles
CX_SPLIT_BLOCKS = 256          # ... and at most this many blocks after the split
GEMM_ROUND_ROWS = 16384        # chunking: whole rounds of the persistent GEMMs


def _cdiv(a, b):
    return -(-a // b)


def _align(n):
    return _cdiv(n, 256) * 256


def scan_segments(S, L, E):
    """-> (G, seg_blocks): segments per strand and 32-step blocks per segment (G == 1: one walk per strand)."""
    waves = S * (E // 64)
    nblk = _cdiv(L, 32)
    long = L >= 2048
    min_blocks = 16 if long else 1
    G = 1
    if L >= 256 and 0 < waves <= (SEG_WAVES_LONG if long else SEG_WAVES_SHORT):
        G = _cdiv(SEG_TARGET_WAVES, waves)
        G = min(G, 8 if long else 16, nblk // min_blocks)
        if G < 3:
            G = 1
    sb = _cdiv(nblk, G)
    return _cdiv(nblk, sb), sb


def scan_pair_wanted(S, L, E):
    waves = S * (E // 64)
    return L % 64 == 0 and L >= 128 and 0 < waves <= PAIR_MAX_WAVES and scan_segments(S, L, E)[0] == 1


def convx_ksplit(S, L, E, bf16):
    """K-split factor of the fused conv + x_proj launch (1: none)."""
    kc = CX_ROWB // (2 if bf16 else 4)
    nkt = E // kc
    tiles = S * _cdiv(L, CX_ROWS)
    if tiles <= 0 or tiles > CX_SPLIT_TILES:
        return 1
    best = 1
    for ks in range(2, nkt // 2 + 1):
        if nkt % ks == 0 and tiles * ks <= CX_SPLIT_BLOCKS:
            best = ks
    return best


def padded_dt_rank(R):
    return 64 if R <= 64 else _cdiv(R, 32) * 32


def chunk_row_limit(E, bf16):
    return ((1 << 32) - (2 << 20)) // (E * (2 if bf16 else 4)) & ~7


def chunk_for(B, L, E, bf16, chunk_seqs=0):
    """Windows per chunk (csrc/api.hip::chunk_for without "workspace_limit_mb")."""
    cap = chunk_row_limit(E, bf16) // (2 * L)
    if 0 < chunk_seqs < cap:
        cap = chunk_seqs
    cap = min(max(cap, 1), B)
    n = _cdiv(B, cap)
    if chunk_seqs == 0:
        def whole(m):
            return (2 * _cdiv(B, m) * L) % GEMM_ROUND_ROWS == 0
        if not whole(n):
            for m in range(n + 1, min(2 * n, B) + 1):
                if whole(m):
                    n = m
                    break
    return _cdiv(B, n)


def predict(D, dt_rank, bf16, B, L, chunk_seqs=0, scan_segments_on=True, expand=2):
    """The forms a pcad_forward call of B windows of L positions runs, and the scratch bytes they carve:
    dict(G, seg_blocks, pair, ks, chunk, scratch)."""
    E = expand * D
    Rp = padded_dt_rank(dt_rank)
    convx = Rp in (64, 96)                     # the fused conv + x_proj kernel (every width here has the blocked layouts)
    S, Sc = 2 * B, 2 * chunk_for(B, L, E, bf16, chunk_seqs)
    G, sb = scan_segments(S, L, E) if scan_segments_on else (1, _cdiv(L, 32))
    pair = scan_segments_on and convx and scan_pair_wanted(S, L, E)
    ks = convx_ksplit(S, L, E, bf16) if scan_segments_on and convx else 1
    scratch = 0
    if G > 1:
        scratch += _align(Sc * G * E * 17 * 4)
    if pair:
        scratch += _align(Sc * E * 256)
    if ks > 1:
        scratch += _align(ks * 2 * Sc * L * (Rp + 32) * 4)
    return dict(G=G, seg_blocks=sb, pair=pair, ks=ks, chunk=Sc // 2, scratch=scratch)


# ---- csrc/gemm.hip: which kernel a GEMM launch runs (launch_gemm_nt / _split / _two / _res -> launch_gemm256_t) ---------------------
GEMM_NT, GEMM_256Q, GEMM_256R = "gemm_nt_kernel 256x128", "gemm256q_kernel 256x256 4-wave", "gemm256r_kernel 256x256 8-wave"
GEMM_TILE = {GEMM_NT: (256, 128), GEMM_256Q: (256, 256), GEMM_256R: (256, 256)}
GEMM_ROWB = 128                # bytes of K per K-tile row: 64 bf16 / 32 fp32 elements


def gemm_quad_ok(M, N, lda, ldw, esz, two=False, nsplit=0):
    """gemm.hip quad_ok: whole 256 x 256 tiles, the two outputs split on a 64-column group, unsigned 32-bit operand offsets"""
    lim = (1 << 32) - 65536
    return M % 256 == 0 and N % 256 == 0 and (not two or nsplit % 64 == 0) and M * lda * esz < lim and N * ldw * esz < lim


def gemm_kernel(form, M, N, esz, lda, ldw, osz=None, ldc=None, nsplit=0, epilogue=False):
    """The kernel a launch of `form` ("plain", "xproj", "two", "residual") runs; None: the launcher refuses it.  esz / osz: operand and
    output element sizes; epilogue: a fused epilogue (the two form's rscale; the residual form always has one)."""
    osz = esz if osz is None else osz
    if form == "xproj":
        return GEMM_NT
    if form == "plain":
        ldc = N if ldc is None else ldc
        big = M >= 2048 and N >= 512 and N % 16 == 0 and (osz == esz or (esz == 2 and osz == 4)) and (ldc * osz) % 16 == 0
        if not big:
            return GEMM_NT
        return GEMM_256Q if gemm_quad_ok(M, N, lda, ldw, esz) else GEMM_256R
    two = form == "two"
    qok = gemm_quad_ok(M, N, lda, ldw, esz, two, nsplit)
    if form == "residual" or epilogue:
        return GEMM_256Q if qok and osz == esz else None       # the fused epilogues exist on the 4-wave kernel only
    return GEMM_256Q if qok else GEMM_256R


def gemm_tiles(kernel, M, N):
    bm, bn = GEMM_TILE[kernel]
    return _cdiv(M, bm) * _cdiv(N, bn)


def gemm_persistent_grid(cu_count, tiles):
    """gemm.hip persistent_grid: one block per CU, a multiple of 8; a block walks tiles b, b + grid, ..."""
    return min(tiles, cu_count // 8 * 8)


def gemm_k_tiles(K, esz):
    """K-tiles per output tile (the split form's K = 3 Ko counts all three passes)"""
    return K * esz // GEMM_ROWB


def _handle(lib, D, n_layer, dt_rank, bf16, opts, expand=2):
    c = engine.PcadConfig(d_model=D, n_layer=n_layer, d_state=16, d_conv=4, expand=expand, dt_rank=dt_rank, vocab=8, eps=1e-5,
                          dtype=1 if bf16 else 0, residual_in_fp32=1, complement=(C.c_int32 * 8)(0, 1, 2, 6, 5, 4, 3, 7))
    h = C.c_void_p()
    assert lib.pcad_create(C.byref(c), C.byref(h)) == 0, lib.pcad_last_error()
    for k, v in opts.items():
        assert lib.pcad_set_option(h, k.encode(), int(v)) == 0, (k, v, lib.pcad_last_error())
    return h


class Probe:
    """Two handles of one geometry and option set, the second with "scan_segments" 0: scratch(B, L) is the library's own
    form scratch for a call of B windows of L positions."""

    def __init__(self, lib, D, dt_rank, bf16, n_layer=2, expand=2, **opts):
        self.lib, self.D, self.dt_rank, self.bf16, self.expand, self.opts = lib, D, dt_rank, bf16, expand, dict(opts)
        self.on = _handle(lib, D, n_layer, dt_rank, bf16, opts, expand)
        self.off = _handle(lib, D, n_layer, dt_rank, bf16, dict(opts, scan_segments=0), expand)

    def scratch(self, B, L):
        a, b = self.lib.pcad_workspace_bytes(self.on, B, L), self.lib.pcad_workspace_bytes(self.off, B, L)
        assert a > 0 and b > 0
        return a - b

    def predict(self, B, L):
        return predict(self.D, self.dt_rank, self.bf16, B, L, chunk_seqs=int(self.opts.get("chunk_seqs", 0)),
                       scan_segments_on=bool(self.opts.get("scan_segments", 1)), expand=self.expand)

    def close(self):
        self.lib.pcad_destroy(self.on)
        self.lib.pcad_destroy(self.off)


def engaged_forms(lib, cfg, B, L, dtype=torch.float32, **opts):
    """The forms a call of B windows of L positions runs on a model of `cfg` (d_model, n_layer, dt_rank, expand) in `dtype` under the
    engine options `opts`, as predicted here - after asserting that the library's scratch bytes equal the prediction.
    -> dict(G, seg_blocks, pair, ks, chunk, scratch)."""
    p = Probe(lib, cfg.d_model, cfg.dt_rank, dtype == torch.bfloat16, n_layer=cfg.n_layer, expand=cfg.expand, **opts)
    try:
        want = p.predict(B, L)
        got = p.scratch(B, L)
    finally:
        p.close()
    assert got == want["scratch"], f"D={cfg.d_model} {dtype} B={B} L={L} {opts}: library scratch {got} != restated {want}"
    return want
