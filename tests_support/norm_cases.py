"""Inputs, launch plans and fp32 emulations of the normalisation kernels, shared by tests/test_gpu_norm_exact.py (which runs the
kernels on these inputs) and tests/test_exact_checker.py (which holds the emulations, sound and with planted faults, to the same
criterion on the CPU).  Everything here is CPU torch; the emulations follow the kernels' summation structure (partials per tile,
then the fixed-order reductions; E[x^2] - mean^2 or centred squares), not their instruction streams."""

import torch

F32, F64 = torch.float32, torch.float64
THREADS, GN_MAX_TILES = 256, 128


# ---- launch plans, restated from the launchers (the GPU tests assert them against sdn_debug_norm_last_launch) ---------------------
def gn16_plan(hw, C):
    """groupnorm_impl's choice for a [hw, C] sample, or None where it returns SDN_E_INVALID."""
    cch = C // 8
    nch = (cch + THREADS - 1) // THREADS
    while cch % nch:
        nch += 1
    ct = cch // nch
    if ct > THREADS:
        return None
    rt = THREADS // ct
    if rt * C * 8 > 64 * 1024:
        return None
    ntiles = min((hw + 31) // 32, GN_MAX_TILES)
    rpt = (hw + ntiles - 1) // ntiles
    return dict(nch=nch, ct=ct, rt=rt, rows_per_tile=rpt, ntiles=(hw + rpt - 1) // rpt)


def gn16_chain(hw, C, G):
    """Longest serial fp32 addition chain of k_gn_stats + k_gn_finalize for one (sample, group): a thread's rows, the group's
    rt x cpg LDS entries, a finalize thread's share of the tiles, the 8 shares, and the division."""
    p = gn16_plan(hw, C)
    return -(-p["rows_per_tile"] // p["rt"]) + p["rt"] * (C // G) + -(-p["ntiles"] // 8) + 8 + 1


def gn16cols_chain(hw, C, G):
    """k_gn_finalize_cols: a thread's share of the (hw / 128) x cpg partials, 6 butterfly steps, 4 waves, the division -- on top of
    the 128 rows each partial itself was summed over."""
    return 128 + -(-(hw // 128) * (C // G) // 256) + 6 + 4 + 1


def ln16_nq_r(C):
    return (1, 4) if C <= 512 else (2, 2) if C <= 1024 else (4, 1)


def ln16_chain(C):
    """k_layernorm / k_row_stats: a lane's NQ x 8 elements, 6 butterfly steps, the division."""
    return 8 * ln16_nq_r(C)[0] + 6 + 1


def lnf32_chain(C):
    return -(-C // 64) + 6 + 1          # k_layernorm_f32: a lane's elements; the register forms add 4 at a time (shorter)


def gnf32_rpc(hw):
    rpc = 16
    while (hw + rpc - 1) // rpc > 64:
        rpc *= 2
    return rpc, (hw + rpc - 1) // rpc


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
OFFSETS, SCALES = (0.5, -0.3), (2.0, 0.7)          # per sample: a wrong sample's statistics are visibly wrong


def affine(C, seed=0, beta0=0.0):
    """(gamma, beta) f32 [C]: 1 + 0.2 N(0, 1) and beta0 + 0.3 N(0, 1).  beta0 = 0 puts the outputs around zero, where y cancels
    against S; the two cases whose clean share is out of fp16's reach there whatever the kernel does (GN16_CASES, GN16_CANCEL)
    also run with beta0 = 3."""
    g = torch.Generator().manual_seed(1000 + seed)
    return 1.0 + 0.2 * torch.randn(C, generator=g), beta0 + 0.3 * torch.randn(C, generator=g)


def gn_input(B, hw, C, dt, seed=0, *, ratio=None, constant=False, near=None, probe_row=None, probe_chunk=None):
    """[B, hw, C] map in dt.  Default: sample b ~ N(OFFSETS[b], SCALES[b]^2).  ratio: |mean| / std of every sample (cancellation
    cases); constant: one value per sample (v = 0); near: values near `near` (fp16 rows near 60000); probe_row / probe_chunk:
    zero everywhere except that row / that 8-channel chunk, so that the row / chunk is all the statistics have."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, hw, C, generator=g)
    sc = torch.tensor([SCALES[b % 2] for b in range(B)]).view(B, 1, 1)
    of = torch.tensor([OFFSETS[b % 2] for b in range(B)]).view(B, 1, 1)
    if ratio is not None:
        x = (z + ratio * torch.sign(of)) * sc
    elif constant:
        x = torch.tensor([1.5, -0.71875][:B] if B <= 2 else [1.5] * B).view(B, 1, 1).expand(B, hw, C).clone()
    elif near is not None:
        x = near + 50.0 * z * torch.sign(of)
    else:
        x = z * sc + of
    if probe_row is not None:
        keep = torch.zeros(hw, dtype=torch.bool); keep[probe_row] = True
        x = torch.where(keep.view(1, hw, 1), x, torch.zeros(()))
    if probe_chunk is not None:
        keep = torch.zeros(C, dtype=torch.bool); keep[8 * probe_chunk:8 * probe_chunk + 8] = True
        x = torch.where(keep.view(1, 1, C), x, torch.zeros(()))
    return x.to(dt)


def ln_input(rows, C, dt, seed=0, *, offset=0.0):
    """[rows, C] in dt: N(0.1, 1.5^2) rows scaled by 2^(i % 5 - 2), plus a common offset (the centred sums' test)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.1) * torch.exp2(torch.arange(rows, dtype=F32) % 5 - 2.0)[:, None]
    return (x + offset).to(dt)


def mod_input(nb, C, seed=0):
    """Stacked adaLN modulation [nb, 3C] = [shift | scale | gate] as the MMDiT passes it (ld_mod = 3C); samples differ visibly."""
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(nb, 3 * C, generator=g) * 0.5 + torch.arange(nb, dtype=F32)[:, None] * 0.25


def mod_rows(mod, C, rows, rows_per_batch):
    """(g, b) [rows, C] of adaLN: 1 + scale and shift of each row's sample."""
    b_of = torch.arange(rows) // rows_per_batch
    return 1.0 + mod[b_of, C:2 * C].double(), mod[b_of, :C].double()


# ---- fp32 emulations ---------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()      # a * b is exact in double; one more rounding than a real fma, rarely


def _silu32(y):
    return y / (1.0 + torch.exp(-y))


def _store(y32, dt, rtz=False):
    if not rtz or dt == F32:
        return y32.to(dt)
    rn = y32.to(dt)
    # round toward zero: where RN went away from zero, step one value of dt back
    away = rn.float().abs() > y32.abs()
    bits = rn.view(torch.int16)
    return torch.where(away, (bits - 1).view(dt), rn)          # sign-magnitude: bits - 1 is the next value toward zero


def _butterfly(s):
    """wave_sum over the last dimension (64 lanes): v += shfl_xor(v, off) for off = 32 ... 1."""
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ off]
    return s


def emulate_gn16_stats(x, G, eps, *, fault=None):
    """(mean, rstd) [B, G] f32 as k_gn_stats + k_gn_finalize leave them in stats_ws.  x [B, hw, C] f32 (the 16-bit values)."""
    B, hw, C = x.shape
    p = gn16_plan(hw, C)
    rt, rpt, nt, cpg = p["rt"], p["rows_per_tile"], p["ntiles"], C // G
    xs = x.clone()
    if fault == "drop_row":
        xs[:, min(rpt, hw - 1)] = 0.0                            # first row of the second tile never accumulated
    k = -(-rpt // rt)
    xp = torch.zeros(B, nt * k * rt, C)                        # zero rows add nothing to an fp32 sum: padding keeps the order
    idx = (torch.arange(nt)[:, None] * rpt + torch.arange(k * rt)[None, :])
    ok = (torch.arange(k * rt)[None, :] < rpt) & (idx < hw)
    xp.view(B, nt, k * rt, C)[:, ok] = xs[:, idx[ok]]
    xp = xp.view(B, nt, k, rt, C)
    s = torch.zeros(B, nt, rt, C); ss = torch.zeros_like(s)
    for kk in range(k):                                         # thread (cl, rl): rows r_lo + rl, + rt, ... in order
        s = s + xp[:, :, kk]
        ss = _fma(xp[:, :, kk], xp[:, :, kk], ss)
    s, ss = s.view(B, nt, rt, G, cpg), ss.view(B, nt, rt, G, cpg)
    gs = torch.zeros(B, nt, G); gq = torch.zeros_like(gs)
    for r in range(rt):                                         # one thread per group: serial over rt x cpg LDS entries
        for c in range(cpg):
            gs = gs + s[:, :, r, :, c]
            gq = gq + ss[:, :, r, :, c]
    pad = (-nt) % 8
    gs = torch.cat([gs, torch.zeros(B, pad, G)], 1).view(B, -1, 8, G)
    gq = torch.cat([gq, torch.zeros(B, pad, G)], 1).view(B, -1, 8, G)
    ps = torch.zeros(B, 8, G); pq = torch.zeros_like(ps)
    for t in range(gs.shape[1]):                                # k_gn_finalize: 8 shares of the tiles, strided
        ps = ps + gs[:, t]; pq = pq + gq[:, t]
    ts = torch.zeros(B, G); tq = torch.zeros_like(ts)
    for j in range(8):
        ts = ts + ps[:, j]; tq = tq + pq[:, j]
    n = torch.tensor(float(hw) * float(cpg))
    mean = ts / n
    var = torch.clamp(tq / (n - 1 if fault == "n_minus_1" else n) - mean * mean, min=0.0)
    rstd = 1.0 / (torch.sqrt(var) + eps) if fault == "eps_outside" else torch.rsqrt(var + eps)
    return mean, rstd


def emulate_gn16(x, G, eps, gamma, beta, silu, dt, *, fault=None):
    """sdn_groupnorm_<dt> on x [B, hw, C] (dt values): (out in dt, mean, rstd).  fault: one of drop_row, next_group_chunk,
    n_minus_1, eps_outside, affine_shift, rtz."""
    B, hw, C = x.shape
    x32 = x.float()
    mean, rstd = emulate_gn16_stats(x32, G, eps, fault=fault)
    cpg = C // G
    gi = torch.arange(C) // cpg
    if fault == "next_group_chunk":                             # the 8-channel chunk that ends group 0 reads group 1's statistics
        c0 = ((cpg - 1) // 8) * 8
        gi = gi.clone(); gi[c0:c0 + 8] = 1
    if fault == "affine_shift":
        gamma, beta = torch.roll(gamma, 1), torch.roll(beta, 1)
    a = rstd[:, gi] * gamma                                     # [B, C]
    cb = beta - mean[:, gi] * a
    y = _fma(x32, a[:, None, :], cb[:, None, :].expand_as(x32))
    if silu:
        y = _silu32(y)
    return _store(y, dt, rtz=fault == "rtz"), mean, rstd


def emulate_ln16(x, g, b, eps, dt, *, mod=False, fault=None, rows_per_batch=0):
    """k_layernorm<T, NQ, R> on x [rows, C]: g, b are gamma, beta [C], or for mod the per-row scale, shift [rows, C] (the kernel
    forms 1 + scale).  Returns (out in dt, mean, rstd) -- mean / rstd are also what k_row_stats writes."""
    rows, C = x.shape
    nq = ln16_nq_r(C)[0]
    x32 = x.float()
    xp = torch.zeros(rows, nq * 512); xp[:, :C] = x32
    live = torch.zeros(nq * 512, dtype=torch.bool); live[:C] = True
    xv, lv = xp.view(rows, nq, 64, 8), live.view(nq, 64, 8)
    s = torch.zeros(rows, 64)
    for q in range(nq):
        for k in range(8):
            s = s + xv[:, q, :, k]
    mean = _butterfly(s)[:, :1] / torch.tensor(float(C))
    ss = torch.zeros(rows, 64)
    for q in range(nq):
        for k in range(8):
            d = torch.where(lv[q, :, k], xv[:, q, :, k] - mean, torch.zeros(()))
            ss = _fma(d, d, ss)
    tot = _butterfly(ss)[:, :1]
    var = tot / torch.tensor(float(C - 1 if fault == "n_minus_1" else C))
    rstd = 1.0 / (torch.sqrt(var) + eps) if fault == "eps_outside" else torch.rsqrt(var + eps)
    if fault == "affine_shift":
        g, b = torch.roll(g, 1, -1), torch.roll(b, 1, -1)
    if fault == "next_sample_scale":                            # the last row of sample 0 is modulated with sample 1's scale
        g = g.clone(); g[rows_per_batch - 1] = g[rows_per_batch]
    gm = (1.0 + g) if mod else g
    y = (x32 - mean) * rstd * gm + b
    return _store(y, dt, rtz=fault == "rtz"), mean[:, 0], rstd[:, 0]


def emulate_gnf32(x, G, eps, gamma, beta, silu):
    """The three f32 GroupNorm forms: statistics in double (E[x^2] - mean^2), rounded to f32; centred apply in f32."""
    B, hw, C = x.shape
    xd = x.double().view(B, hw, G, C // G)
    mean = xd.mean((1, 3))
    var = torch.clamp((xd * xd).mean((1, 3)) - mean * mean, min=0.0)
    mean32, rstd32 = mean.float(), (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=F32)))).float()
    gi = torch.arange(C) // (C // G)
    y = (x - mean32[:, None, gi]) * rstd32[:, None, gi] * gamma + beta
    return _silu32(y) if silu else y


def emulate_lnf32(x, g, b, eps, *, mod=False):
    """k_layernorm_f32 / _regs / _mod_f32: a lane's strided elements, butterfly, centred squares, all f32."""
    rows, C = x.shape
    n = -(-C // 64)
    xp = torch.zeros(rows, n * 64); xp[:, :C] = x
    live = (torch.arange(n * 64) < C).view(n, 64)
    xv = xp.view(rows, n, 64)
    s = torch.zeros(rows, 64)
    for i in range(n):
        s = s + xv[:, i]
    mean = _butterfly(s)[:, :1] / torch.tensor(float(C))
    ss = torch.zeros(rows, 64)
    for i in range(n):
        d = torch.where(live[i], xv[:, i] - mean, torch.zeros(()))
        ss = _fma(d, d, ss)
    rstd = 1.0 / torch.sqrt(_butterfly(ss)[:, :1] / torch.tensor(float(C)) + eps)
    return (x - mean) * rstd * ((1.0 + g) if mod else g) + b


# ---- case tables (the GPU tests run them; the CPU checker derives the hard bounds of STAT from the same shapes) ---------------------
# 16-bit GroupNorm, own statistics pass: name -> shape and the launch plan the case is written for (asserted against the record).
# cancel: a set of ONE element is a constant map (v = 0, y = b exactly, S / |y| ~ 2 |x| / sqrt(eps)): a cancellation case.
# family gn16serial: at G = 1, C = 64 the one thread that reduces a group's rt x cpg LDS partials runs a 2048-term serial fp32 chain
# (every other shape: <= 241); its statistics are measured 7x less accurate and get their own STAT (exact.py).  With that constant
# an fp16 output near zero is no longer decided by its rounding (clean share 0.94 at beta ~ 0), so the case asserts the
# share with beta0 = 3 and runs once more at beta ~ 0 with everything but the share (no_share).
GN16_CASES = {
    "smallest set: hw 1, cpg 1": dict(hw=1, C=32, G=32, cancel=True, plan=dict(nch=1, ct=4, ntiles=1, rows_per_tile=1)),
    "ragged tile: hw 33, C 320, cpg 10, rt 6": dict(hw=33, C=320, G=32, plan=dict(nch=1, ct=40, ntiles=2, rows_per_tile=17)),
    "tile cap: hw 4097 -> 33 rows per tile": dict(hw=4097, C=64, G=32, plan=dict(nch=1, ct=8, ntiles=125, rows_per_tile=33)),
    "uneven tiles: hw 100, G 1": dict(hw=100, C=64, G=1, family="gn16serial", beta0=3.0, plan=dict(nch=1, ct=8, ntiles=4, rows_per_tile=25)),
    "uneven tiles: hw 100, G 1, beta 0": dict(hw=100, C=64, G=1, family="gn16serial", no_share=True, plan=dict(nch=1, ct=8, ntiles=4, rows_per_tile=25)),
    "uneven tiles: hw 100, G 64 (cpg 1)": dict(hw=100, C=64, G=64, plan=dict(nch=1, ct=8, ntiles=4, rows_per_tile=25)),
    "two sources 320 + 640, seam inside group 10": dict(hw=33, C=960, c1=320, G=32, plan=dict(nch=1, ct=120, ntiles=2, rows_per_tile=17)),
    "two channel passes: 1280 + 1280": dict(hw=33, C=2560, c1=1280, G=32, plan=dict(nch=2, ct=160, ntiles=2, rows_per_tile=17)),
    "widest: C 4096": dict(hw=33, C=4096, G=32, plan=dict(nch=2, ct=256, ntiles=2, rows_per_tile=17)),
    "prime chunk count: C 1928 (241 chunks), G 8": dict(hw=33, C=1928, G=8, plan=dict(nch=1, ct=241, ntiles=2, rows_per_tile=17)),
}
GN16_VARIANTS = ((0, 1e-5), (1, 1e-5), (0, 1e-6), (1, 1e-6))          # (silu, eps)
# probe inputs: x = 0 except one row -- first / last row of a tile, first row of the next, last row of the map, and the rows a
# thread reaches only in the partial last 4 * rt stride -- or except one 8-channel chunk at a group edge / the source seam
GN16_ROW_PROBES = {
    "tile cap: hw 4097 -> 33 rows per tile": (0, 32, 33, 4095, 4096),
    "ragged tile: hw 33, C 320, cpg 10, rt 6": (0, 12, 15, 16, 17, 32),
}
GN16_CHUNK_PROBES = {"two sources 320 + 640, seam inside group 10": (3, 39, 40, 119)}
# cancellation cases (named: exempt from the clean share, except ratio 3): gn_input keywords
# "|mean| / std 3" must meet the clean share; with beta ~ 0 fp16 cannot for ANY kernel (S carries |mu| = 3 sigma: 0.975 at
# STAT = 2^-20), so it runs with beta0 = 3 (share asserted) and, as "..., beta 0", at beta ~ 0 (bound asserted, share recorded).
GN16_CANCEL = {
    "|mean| / std 3": dict(ratio=3.0, beta0=3.0), "|mean| / std 3, beta 0": dict(ratio=3.0), "|mean| / std 30": dict(ratio=30.0), "|mean| / std 100": dict(ratio=100.0),
    "constant map (v = 0)": dict(constant=True), "fp16 rows near 60000": dict(near=60000.0),
}
GN16_COLS_CASES = {
    "column sums: hw 128, C 320": dict(hw=128, C=320, G=32), "column sums: hw 384, C 320": dict(hw=384, C=320, G=32),
    "column sums: hw 128, 320 + 640": dict(hw=128, C=960, c1=320, G=32), "column sums: hw 384, 320 + 640": dict(hw=384, C=960, c1=320, G=32),
}
LN16_WIDTHS = (8, 320, 512, 520, 768, 1024, 1032, 1536, 2048)


def ln16_rows(C):
    """rows = 1, 4R k + 1, 4R k - 1 (k = 2) for the width's R: a lone row, one row into the next workgroup, one row short of it."""
    r = ln16_nq_r(C)[1]
    return (1, 8 * r + 1, 8 * r - 1)


GNF32_ROWS_CASES = {           # row-major form: (hw, C, c1, G) -> (rpc, nchunk) by gnf32_rpc
    "rows: hw 1, C 32": dict(hw=1, C=32, G=32), "rows: hw 17, 320 + 640": dict(hw=17, C=960, c1=320, G=32),
    "rows: hw 17, C 2560, G 64": dict(hw=17, C=2560, G=64), "rows: hw 1025 (33 chunks, last 1 row), 320 + 640, G 64": dict(hw=1025, C=960, c1=320, G=64),
    "rows: hw 2049 (rpc doubled twice), C 32": dict(hw=2049, C=32, G=32), "rows: hw 1, C 2560": dict(hw=1, C=2560, G=32),
}
GNF32_PAIRS_CASES = {          # k_groupnorm_f32: stats_ws = NULL, or C > GN_MAXC
    "pairs: cpg 2 (hp 1)": dict(hw=37, C=64, G=32), "pairs: cpg 6 (hp 3, dead threads)": dict(hw=37, C=192, G=32),
    "pairs: cpg 10 (hp 5, dead threads)": dict(hw=37, C=320, G=32), "pairs: cpg 512 (hp 256)": dict(hw=37, C=1024, G=2),
    "pairs: 324 + 316, even seam inside group 32": dict(hw=37, C=640, c1=324, G=64),
    "pairs: C 2564 > GN_MAXC with a workspace": dict(hw=5, C=2564, G=641, ws=True),
}
GNF32_ANY_CASES = {            # k_groupnorm_f32_any
    "any: cpg 3": dict(hw=37, C=96, G=32), "any: cpg 1024 > 512": dict(hw=37, C=2048, G=2), "any: odd c1 5 + 3": dict(hw=37, C=8, c1=5, G=2),
    "any: x 4 bytes off 8-byte alignment": dict(hw=37, C=64, G=32, misalign=True),
}
LNF32_REGS_WIDTHS, LNF32_GENERIC_WIDTHS = (4, 260, 1280), (77, 1284, 1538)
LNF32_MOD_WIDTHS = {512: 2, 516: 4, 1024: 4, 1028: 8, 2048: 8}          # width -> NV


def stat_chains():
    """Longest serial fp32 chain of each family's statistics over the tested shapes: x 2^-24 = the hard bound of its STAT.
    The f32 GroupNorm forms accumulate in double and round mean and rstd to f32 once each: 2^-24 m1 on the mean, 2^-24 r on rstd,
    which is at most 2 x 2^-24 in STAT's unit r M2 / (2 (v + eps)) >= r / 2 (eps << v): chain 2."""
    gn = max(gn16_chain(c["hw"], c["C"], c["G"]) for c in GN16_CASES.values() if c.get("family", "gn16") == "gn16")
    serial = max(gn16_chain(c["hw"], c["C"], c["G"]) for c in GN16_CASES.values() if c.get("family") == "gn16serial")
    cols = max(gn16cols_chain(c["hw"], c["C"], c["G"]) for c in GN16_COLS_CASES.values())
    ln = max(ln16_chain(C) for C in LN16_WIDTHS)
    lnf = max(lnf32_chain(C) for C in LNF32_REGS_WIDTHS + LNF32_GENERIC_WIDTHS + tuple(LNF32_MOD_WIDTHS))
    return {"gn16": gn, "gn16serial": serial, "gn16cols": cols, "ln16": ln, "gnf32": 2, "lnf32": lnf}
