"""Reference of the geodesic scribble expansion (include/pacingpseudo_geo.h has the definition), written from that definition: a
numpy float32 heap Dijkstra with the cost formula rounded operation by operation, whole-plane sweep relaxation in a chosen
neighbour order (the Dijkstra's own check), the float64 normalisation and the label rule.  Nothing here is shared with the kernels."""
import heapq

import numpy as np

F = np.float32
AXIS, DIAG = F(1.0), np.frombuffer(np.uint32(0x3FB504F3).tobytes(), dtype=np.float32)[0]
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
INF = F(np.inf)


def normalise(img):
    """The guide of one slice in float64, rounded to fp32 once."""
    img = np.asarray(img, dtype=np.float64)
    return ((img - img.mean()) / (img.std() + 1e-8)).astype(np.float32)


def step_cost(gp, gq, dy, dx, lam):
    """c(p, q) = fl(s + fl(lam |fl(g_p - g_q)|)); scalars or arrays of float32."""
    with np.errstate(invalid='ignore', over='ignore'):
        s = DIAG if (dy != 0 and dx != 0) else AXIS
        return F(s + F(F(lam) * np.abs(F(F(gp) - F(gq)))))


def dijkstra(g, seeds, lam):
    """dist (h, w) float32 of one class: `seeds` a boolean (h, w) map.  +inf everywhere without a seed."""
    g = np.asarray(g, dtype=np.float32)
    h, w = g.shape
    d = np.full((h, w), INF, dtype=np.float32)
    heap = []
    for y, x in zip(*np.nonzero(seeds)):
        d[y, x] = F(0)
        heap.append((0.0, int(y), int(x)))
    heapq.heapify(heap)
    lam = F(lam)
    done = np.zeros((h, w), dtype=bool)
    with np.errstate(invalid='ignore', over='ignore'):
        while heap:
            dp, y, x = heapq.heappop(heap)
            if done[y, x] or dp != d[y, x]:
                continue
            done[y, x] = True
            gp = g[y, x]
            for dy, dx in NEIGHBOURS:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and not done[yy, xx]:
                    s = DIAG if (dy and dx) else AXIS
                    cand = F(d[y, x] + F(s + F(lam * np.abs(F(gp - g[yy, xx])))))
                    if cand < d[yy, xx]:
                        d[yy, xx] = cand
                        heapq.heappush(heap, (float(cand), yy, xx))
    return d


def sweep_relaxation(g, seeds, lam, order=NEIGHBOURS, max_sweeps=100000):
    """(dist, sweeps): Jacobi-free whole-plane relaxation -- every sweep lowers each pixel IN PLACE from one neighbour direction
    after the other, in `order` -- until a sweep changes nothing.  `sweeps` counts the sweeps that changed something."""
    g = np.asarray(g, dtype=np.float32)
    h, w = g.shape
    d = np.where(seeds, F(0), INF).astype(np.float32)
    lam = F(lam)
    sweeps = 0
    with np.errstate(invalid='ignore', over='ignore'):
        for _ in range(max_sweeps):
            changed = False
            for dy, dx in order:                      # q = p + (dy, dx): the source p is q - (dy, dx)
                qy = slice(max(dy, 0), h + min(dy, 0))
                qx = slice(max(dx, 0), w + min(dx, 0))
                py = slice(max(-dy, 0), h + min(-dy, 0))
                px = slice(max(-dx, 0), w + min(-dx, 0))
                cand = (d[py, px] + step_cost(g[py, px], g[qy, qx], dy, dx, lam)).astype(np.float32)
                low = cand < d[qy, qx]
                if low.any():
                    d[qy, qx] = np.where(low, cand, d[qy, qx])
                    changed = True
            if not changed:
                return d, sweeps
            sweeps += 1
    raise RuntimeError('sweep relaxation did not converge')


def distances(g, scb, K, lam):
    """dist (K, h, w) float32 of one slice from its guide and scribble map (values 0 .. K)."""
    scb = np.asarray(scb)
    return np.stack([dijkstra(g, scb == k, lam) for k in range(K)])


def labels(dist, scb, K, ratio=0.25, max_dist=np.inf):
    """The ratio rule on dist (K, h, w): int64 (h, w)."""
    dist, scb = np.asarray(dist, dtype=np.float32), np.asarray(scb)
    arg = dist.argmin(0)                               # the first minimum
    best = np.take_along_axis(dist, arg[None], 0)[0]
    rest = dist.copy()
    np.put_along_axis(rest, arg[None], INF, 0)
    second = rest.min(0)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(best) & (best <= F(max_dist)) & (best <= (F(ratio) * second).astype(np.float32))
    out = np.where(ok, arg, K)
    return np.where((scb >= 0) & (scb < K), scb, out).astype(np.int64)


def spiral_maze(size=67, wall=100.0):
    """(guide, seeds): a one-pixel corridor of 0 spiralling inwards between walls of `wall`, the seed at its outer end (0, 0)."""
    g = np.full((size, size), wall, dtype=np.float32)
    y = x = 0
    dy, dx = 0, 1
    lo_y, hi_y, lo_x, hi_x = 0, size - 1, 0, size - 1
    g[0, 0] = 0.0
    while True:
        moved = False
        while lo_y <= y + dy <= hi_y and lo_x <= x + dx <= hi_x:
            y, x = y + dy, x + dx
            g[y, x] = 0.0
            moved = True
        if not moved:
            break
        if (dy, dx) == (0, 1):
            lo_y += 2
        elif (dy, dx) == (1, 0):
            hi_x -= 2
        elif (dy, dx) == (0, -1):
            hi_y -= 2
        else:
            lo_x += 2
        dy, dx = dx, -dy
    seeds = np.zeros((size, size), dtype=bool)
    seeds[0, 0] = True
    return g, seeds


def comb_maze(h=33, w=130, wall=100.0):
    """(guide, seeds): odd rows hold a wall with a single gap that alternates between x = w - 1 and x = 0; the seed at (0, 0)."""
    g = np.zeros((h, w), dtype=np.float32)
    for i, y in enumerate(range(1, h, 2)):
        g[y, :] = wall
        g[y, w - 1 if i % 2 == 0 else 0] = 0.0
    seeds = np.zeros((h, w), dtype=bool)
    seeds[0, 0] = True
    return g, seeds


def phantom(seed, size=32, K=5):
    """(img, lab, scb) of SyntheticPhantoms(1, K, size, seed=seed, raw=True)[0]."""
    from pacingpseudo_amd.data import SyntheticPhantoms
    d = SyntheticPhantoms(1, K, size=size, seed=seed, raw=True)[0]
    return d['img'], d['lab'], d['scb']
