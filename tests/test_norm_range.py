"""The mean-to-spread envelope of the normalisation statistics, derived on the CPU (docs/norm_range.md).

Every train-mode statistic of this tree is the one-pass  var = sum z^2 / n - (sum z / n)^2  with fp32 partial sums below and double
above.  Its error grows with r = |mean| / sigma (like r^2 times the relative error of sum z^2) and with the number of values one
fp32 partial holds.  This file restates, in numpy, the plan and the summation order of every producer:
  col_plan                  pp_norm.hip: c4, rows, chunk, nblk of a streaming launch; chunk / rows values per fp32 partial;
  stream_sums               bn_stats_partial_kernel: per thread s += v, q = fma(v, v, q) in fp32, in pixel order; the rows of a
                            block, then the blocks, in double (fin_reduce2 / bn_reduce_partials_kernel);
  epilogue_sums             the fused epilogues of pp_conv.hip / pp_wino.hip: a tile partial of `tile` values per lane in fp32, the
                            tiles of a lane in fp32, two lanes folded in fp32 (__shfl_xor), everything above in double;
  finalize                  bn_stats_finalize_kernel: mean, var in double, var clamped at 0, (float)var, 1 / sqrtf(varf + eps),
                            scale and shift in fp32, the unbiased running update in fp32;
  gn_rows                   gn_stats_finalize_kernel: the channels of a group folded in double, then the same arithmetic;
and derives the DECLARED ENVELOPE from them: for a bound b in (TOL_SUMS, TOL), r_b is the largest power of two up to which the
worst emulated error of the rows save_invstd, scale, shift, running_var -- over 16 seeded draws of 8 channels, the depths 8, 64 and
256 and the producers above, relative to the row maximum as the census measures (_rel) -- stays within b / 4.  The factor 4 is the
margin for a summation order on the device that the emulation only approximates.  tests/test_gpu_norm_range.py imports the
envelope from here and holds the kernels to it on the MI355X; nothing in this file runs on a GPU.
"""
import functools

import numpy as np

TOL, TOL_SUMS = 1e-4, 1e-5          # tests/test_gpu_conv_census.py (asserted equal in tests/test_gpu_norm_range.py)
EPS, MOM = 1e-5, 0.1
NORM_THREADS, BLOCKS = 256, 512
DEPTHS = (8, 64, 256)
MARGIN = 4.0
ROWS = ('save_invstd', 'scale', 'shift', 'running_var')
SEEDS, CHANNELS, THREADS = 16, 8, 512          # THREADS: partials per channel of a rows = 1 launch (512 blocks), the fewest there are
f32, f64 = np.float32, np.float64


def _cdiv(a, b):
    return -(-a // b)


def col_plan(C, ppg, groups):
    """(c4, rows, chunk, nblk) of col_plan (pp_norm.hip)"""
    c4 = C // 4
    rows = max(NORM_THREADS // c4, 1)
    target = max(BLOCKS // groups, 1)
    chunk = max(_cdiv(ppg, target), rows * 8)
    chunk = _cdiv(chunk, rows) * rows
    return c4, rows, chunk, _cdiv(ppg, chunk)


def depth(C, ppg, groups):
    """values per fp32 partial of a streaming BatchNorm launch"""
    _, rows, chunk, _ = col_plan(C, ppg, groups)
    return chunk // rows


def bn_workspace(C, ppg, groups):
    """pp_bn_workspace"""
    return groups * col_plan(C, ppg, groups)[3] * 2 * C * 8 + 256


def pixels_for_depth(C, groups, d):
    """the fewest pixels per group at which every thread of a full launch (512 blocks) holds d values per channel"""
    rows = col_plan(C, 1, 1)[1]
    assert (d * rows * BLOCKS) % groups == 0
    return d * rows * BLOCKS // groups


# ------------------------------------------------------------------------------------------------------------- summation orders
def _fma(q, v):
    """fp32 fma(v, v, q): the product of two fp32 numbers is exact in double"""
    return (q.astype(f64) + v.astype(f64) * v.astype(f64)).astype(f32)


def stream_sums(z):
    """z (..., threads, depth) fp32 -> (sum, sum of squares) float64 (...): bn_stats_partial_kernel and the reductions above it"""
    s, q = np.zeros(z.shape[:-1], f32), np.zeros(z.shape[:-1], f32)
    for j in range(z.shape[-1]):
        v = z[..., j]
        s = s + v
        q = _fma(q, v)
    return s.astype(f64).sum(-1), q.astype(f64).sum(-1)


def epilogue_sums(z, tile=16):
    """z (..., lanes, depth) fp32, depth a multiple of tile -> (sum, sum of squares) float64: a fused epilogue's order"""
    s, q = np.zeros(z.shape[:-1], f32), np.zeros(z.shape[:-1], f32)
    for t in range(z.shape[-1] // tile):
        ts, tq = np.zeros_like(s), np.zeros_like(q)
        for j in range(tile):
            v = z[..., t * tile + j]
            ts = ts + v
            tq = _fma(tq, v)
        s, q = s + ts, q + tq
    s, q = s[..., 0::2] + s[..., 1::2], q[..., 0::2] + q[..., 1::2]          # the two lanes of a channel, __shfl_xor
    return s.astype(f64).sum(-1), q.astype(f64).sum(-1)


def finalize(s, q, n, gamma, beta, rv, eps=EPS, mom=MOM):
    """bn_stats_finalize_kernel on double sums: fp32 rows save_mean, save_invstd, scale, shift, running_var, and var (double)"""
    mean = s / n
    var = np.maximum(q / n - mean * mean, 0.0)
    meanf, varf = mean.astype(f32), var.astype(f32)
    invstd = f32(1.0) / np.sqrt(varf + f32(eps))
    sc = invstd * gamma.astype(f32)
    shift = (beta.astype(f64) - meanf.astype(f64) * sc.astype(f64)).astype(f32)           # one rounding: the compiler contracts it
    unbiased = (var * (n / (n - 1.0 if n > 1 else 1.0))).astype(f32)
    rvn = f32(1.0 - f32(mom)) * rv.astype(f32) + f32(mom) * unbiased
    return {'save_mean': meanf, 'save_invstd': invstd, 'scale': sc, 'shift': shift, 'running_var': rvn, 'var': var}


def gn_rows(s, q, hw, cpg, gamma, beta, eps=EPS):
    """gn_stats_finalize_kernel: s, q (..., C) double per channel -> fp32 rows per channel"""
    m = float(cpg * hw)
    sg = s.reshape(s.shape[:-1] + (-1, cpg)).sum(-1, keepdims=True)
    qg = q.reshape(q.shape[:-1] + (-1, cpg)).sum(-1, keepdims=True)
    mean = sg / m
    var = np.maximum(qg / m - mean * mean, 0.0)
    meanf = mean.astype(f32)
    invstd = f32(1.0) / np.sqrt(var.astype(f32) + f32(eps))
    expand = lambda t: np.broadcast_to(t, t.shape[:-1] + (cpg,)).reshape(s.shape)          # noqa: E731
    meanf, invstd = expand(meanf), expand(invstd)
    sc = invstd * gamma.astype(f32)
    return {'save_mean': meanf, 'save_invstd': invstd, 'scale': sc,
            'shift': (beta.astype(f64) - meanf.astype(f64) * sc.astype(f64)).astype(f32), 'var': expand(var)}


def reference(z, gamma, beta, rv, eps=EPS, mom=MOM):
    """float64, two passes, of the same fp32 values: z (..., C, n)"""
    z = z.astype(f64)
    n = z.shape[-1]
    mean = z.mean(-1)
    var = ((z - mean[..., None]) ** 2).mean(-1)
    invstd = 1.0 / np.sqrt(var + eps)
    sc = gamma * invstd
    return {'save_mean': mean, 'save_invstd': invstd, 'scale': sc, 'shift': beta - mean * sc,
            'running_var': (1 - mom) * rv + mom * var * n / (n - 1)}


def gn_reference(z, cpg, gamma, beta, eps=EPS):
    """z (..., C, n) -> float64 rows per channel of a GroupNorm with cpg channels per group"""
    z = z.astype(f64)
    zg = z.reshape(z.shape[:-2] + (-1, cpg * z.shape[-1]))
    mean = zg.mean(-1, keepdims=True)
    var = ((zg - mean) ** 2).mean(-1, keepdims=True)
    expand = lambda t: np.broadcast_to(t, t.shape[:-1] + (cpg,)).reshape(z.shape[:-1])        # noqa: E731
    mean, invstd = expand(mean), expand(1.0 / np.sqrt(var + eps))
    sc = gamma * invstd
    return {'save_mean': mean, 'save_invstd': invstd, 'scale': sc, 'shift': beta - mean * sc}


def rel(got, ref):
    """_rel of the census, per draw: max |got - ref| over the channels of a row, relative to the row maximum"""
    return np.abs(got.astype(f64) - ref).max(-1) / (np.abs(ref).max(-1) + 1e-30)


# --------------------------------------------------------------------------------------------------------------------- draws
@functools.lru_cache(maxsize=None)
def _normals(d, seed):
    """(CHANNELS, THREADS, d) standard normal fp32 and the per-channel sigma, gamma, beta, running variance of one seeded draw"""
    rng = np.random.default_rng(1000 * d + seed)
    g = rng.standard_normal((CHANNELS, THREADS, d), dtype=f32)
    sig = (rng.random(CHANNELS) * 1.5 + 0.5).astype(f32)
    gamma = (rng.random(CHANNELS) + 0.5).astype(f32)
    gamma[0] = -0.7
    return g, sig, gamma, rng.standard_normal(CHANNELS).astype(f32), (rng.random(CHANNELS) + 0.5).astype(f32)


def draw(r, d, seed, k=0):
    """z = (sigma_c * randn +- r * sigma_c) * 2^k in fp32, as _DOps.norm_z under NormProfile(offset=r, scale=k) draws it"""
    g, sig, gamma, beta, rv = _normals(d, seed)
    sign = (1.0 - 2.0 * (np.arange(CHANNELS) % 2)).astype(f32)
    z = g * sig[:, None, None] + (f32(r) * sig * sign)[:, None, None]
    return z * f32(2.0 ** k), gamma, beta, rv * (sig * f32(2.0 ** k)) ** 2


PRODUCERS = ('stream', 'epilogue', 'gn')


@functools.lru_cache(maxsize=None)
def errors(r, d, k=0):
    """{producer: {row: worst relative error over the seeded draws}} of the emulations at mean-to-spread ratio r, depth d; with
    'clamped': whether the variance of a channel came out as 0"""
    out = {p: dict.fromkeys(ROWS, 0.0) for p in PRODUCERS}
    n = THREADS * d
    for seed in range(SEEDS):
        z, gamma, beta, rv = draw(r, d, seed, k)
        flat = z.reshape(CHANNELS, n)
        g64, b64 = gamma.astype(f64), beta.astype(f64)
        ref, gref = reference(flat, g64, b64, rv.astype(f64)), gn_reference(flat, 4, g64, b64)
        ss, sq = stream_sums(z)
        es, eq = epilogue_sums(z) if d % 16 == 0 else (ss, sq)         # (a depth below the tile: one tile partial, the same order)
        for p, got, want in (('stream', finalize(ss, sq, float(n), gamma, beta, rv), ref),
                             ('epilogue', finalize(es, eq, float(n), gamma, beta, rv), ref),
                             ('gn', gn_rows(ss, sq, n, 4, gamma, beta), gref)):          # four channels per group, offsets differing
            for row in ROWS:
                if row in want:
                    out[p][row] = max(out[p][row], float(rel(got[row], want[row])))
            out[p]['clamped'] = out[p].get('clamped', False) or bool((got['var'] == 0).any())
    return out


def worst(r, d=None, producers=PRODUCERS, k=0):
    """the largest emulated error of the rows ROWS at ratio r: over the producers and the depths (or the one given)"""
    return max(errors(r, dd, k)[p][row] for p in producers for dd in (DEPTHS if d is None else (d,)) for row in ROWS)


@functools.lru_cache(maxsize=None)
def envelope():
    """(r_TOL_SUMS, r_TOL): per bound the largest power of two up to which every power of two holds bound / MARGIN"""
    out = []
    for bound in (TOL_SUMS, TOL):
        r = 0
        while r < 4096 and worst(max(2 * r, 1)) <= bound / MARGIN:
            r = max(2 * r, 1)
        out.append(r)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------- tests
def test_col_plan_mirrors_the_kernel_file():
    """Two rows computed by hand from col_plan (pp_norm.hip).  The widest tensors of the workload, 32 channels of 2 x 32 x 256^2
    pixels in two groups: c4 = 8, rows = 256 / 8 = 32, target = 512 / 2 = 256 blocks, chunk = 2097152 / 256 = 8192 (a multiple
    of rows, above the floor 8 * rows = 256), nblk = 256, depth 8192 / 32 = 256.  The idle-lane row of NORM_EDGES, 516 channels
    of 300 pixels: c4 = 129, rows = 256 / 129 = 1, chunk = ceil(300 / 512) = 1 raised to the floor 8, nblk = ceil(300 / 8) = 38."""
    assert col_plan(32, 2097152, 2) == (8, 32, 8192, 256) and depth(32, 2097152, 2) == 256
    assert col_plan(516, 300, 1) == (129, 1, 8, 38) and depth(516, 300, 1) == 8
    # NORM_EDGES' largest row is at the floor too: chunk = max(ceil(49425 / 512) = 97, 256) = 256, depth 8
    assert col_plan(32, 49425, 1) == (8, 32, 256, 194) and depth(32, 49425, 1) == 8
    assert bn_workspace(32, 2097152, 2) == 2 * 256 * 2 * 32 * 8 + 256
    for C, G, d in ((32, 2, 64), (64, 1, 64), (1024, 1, 64), (516, 1, 64), (32, 2, 256)):
        P = pixels_for_depth(C, G, d)
        assert depth(C, P, G) == d and col_plan(C, P, G)[3] == BLOCKS // G, (C, G, d)
    assert pixels_for_depth(32, 2, 256) == 2097152


def test_summation_orders_are_exact_where_they_must_be():
    """A constant channel sums exactly (0.5 and 0.25 are powers of two, the counts stay below 2^24): variance exactly 0, and
    invstd = 1 / sqrtf(eps), as the census requires of its last channel; small integers sum exactly in either order."""
    z = np.full((1, 64, 256), 0.5, f32)
    for sums in (stream_sums, epilogue_sums):
        s, q = sums(z)
        row = finalize(s, q, 64.0 * 256, np.ones(1, f32), np.zeros(1, f32), np.ones(1, f32))
        assert row['var'][0] == 0.0 and row['save_mean'][0] == 0.5
        assert row['save_invstd'][0] == f32(1.0) / np.sqrt(f32(EPS))
    ints = np.random.default_rng(1).integers(-8, 9, (3, 32, 64)).astype(f32)
    for sums in (stream_sums, epilogue_sums):
        s, q = sums(ints)
        assert np.array_equal(s, ints.astype(f64).sum((1, 2))) and np.array_equal(q, (ints.astype(f64) ** 2).sum((1, 2)))


def test_declared_envelope():
    """The envelope by the stated rule, and the emulation asserted at the declared points."""
    r_sums, r_tol = envelope()
    print(f'\ndeclared envelope: r_TOL_SUMS = {r_sums}, r_TOL = {r_tol}')
    assert 1 <= r_sums <= r_tol
    for r in (0, 1, r_sums):
        assert worst(r) <= TOL_SUMS / MARGIN, (r, worst(r))
    assert worst(r_tol) <= TOL / MARGIN, (r_tol, worst(r_tol))
    assert worst(2 * r_sums) > TOL_SUMS / MARGIN and worst(2 * r_tol) > TOL / MARGIN          # the largest such powers of two


def test_the_bound_is_not_vacuous():
    """At r = 256 and depth 256 the emulated streaming statistics miss TOL: the formulation has an edge and the bound sees it."""
    e = errors(256, 256)['stream']
    print(f'\nr = 256, depth 256: ' + ', '.join(f'{row} {e[row]:.3g}' for row in ROWS))
    assert max(e[row] for row in ROWS) > TOL, e


def test_scale_leaves_the_relative_error_alone_until_eps_takes_over():
    """z * 2^k: every fp32 operation of the sums scales exactly, so mean and var carry the same relative error; at k = -10 the
    variance (~1e-6) lies below eps and invstd is ~1 / sqrt(eps), at k = +10 eps is negligible.  Both hold TOL_SUMS / MARGIN."""
    r_sums, _ = envelope()
    for k in (-10, 10):
        for d in DEPTHS:
            assert worst(r_sums, d, ('stream', 'gn'), k) <= TOL_SUMS / MARGIN, (k, d, errors(r_sums, d, k))


def _invstd_error(z, gamma, beta, rv):
    n = z.shape[1] * z.shape[2]
    s, q = stream_sums(z)
    ref = reference(z.reshape(z.shape[0], n), gamma.astype(f64), beta.astype(f64), rv.astype(f64))
    return float(rel(finalize(s, q, float(n), gamma, beta, rv)['save_invstd'], ref['save_invstd']))


def test_fp16_storage_drifts_where_bf16_adds_exactly():
    """What the GPU shows for pp_bn_train_stats_h16 at r = 8, depth 64 (0.85 of TOL_SUMS against 0.02 for an fp32 operand) is a
    property of the data, and the emulation has it too.  Near 8 sigma the fp16 grid is 2^-7, the squares are multiples of 2^-14,
    and against the ulp 2^-11 of a partial between 4096 and 8192 their residues are 0, 1/8 or 1/2 only: round-to-nearest drops the
    1/8 every time, a drift instead of a random walk.  bf16 squares are whole ulps of the partial.  The declared envelope is
    derived for fp32 operands; this only pins the direction of the effect."""
    import torch
    err = {'fp32': 0.0, 'fp16': 0.0, 'bf16': 0.0}
    for seed in range(4):
        z, gamma, beta, rv = draw(8, 64, seed)
        err['fp32'] = max(err['fp32'], _invstd_error(z, gamma, beta, rv))
        err['fp16'] = max(err['fp16'], _invstd_error(z.astype(np.float16).astype(f32), gamma, beta, rv))
        err['bf16'] = max(err['bf16'], _invstd_error(torch.from_numpy(z).bfloat16().float().numpy(), gamma, beta, rv))
    print(f'\nr = 8, depth 64, save_invstd: ' + ', '.join(f'{k} {v:.3g}' for k, v in err.items()))
    assert err['fp16'] > 4 * err['fp32'] and err['bf16'] <= err['fp32'], err


def table(out=None):
    """The emulation table of docs/norm_range.md: worst error of the rows ROWS per producer and depth"""
    rs = (1, 2, 4, 8, 16, 32, 64, 128, 256)
    print('| producer | depth | ' + ' | '.join(f'r={r}' for r in rs) + ' |\n|---|---|' + '---|' * len(rs), file=out)
    for p in PRODUCERS:
        for d in DEPTHS:
            print(f'| {p} | {d} | ' + ' | '.join(f'{worst(r, d, (p,)):.2g}' for r in rs) + ' |', file=out)
    print(f'\ndeclared envelope: r_TOL_SUMS = {envelope()[0]}, r_TOL = {envelope()[1]}', file=out)


if __name__ == '__main__':
    table()
