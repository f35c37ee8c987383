"""numpy / scipy restatement of the two definitions of include/pacingpseudo_morph.h ("Size threshold and hole
filling"), one item -- an (H, W) slice or a (D, H, W) volume -- at a time.  Written from the definitions, not from the kernels:
ndimage.label per class and bincount for the threshold; ndimage.label of cm == 0, a border test and a dilated ring per cavity for
the hole filling.  Nothing here runs on a device."""
import numpy as np
from scipy import ndimage


def structure(ndim, connectivity):
    return ndimage.generate_binary_structure(ndim, connectivity)


def _thresholds(min_size, K):
    return [int(min_size)] * K if np.isscalar(min_size) else [int(s) for s in min_size]


def remove_small(cm, K, min_size, connectivity=1):
    """-> (out, stats (K, 2) int32 = {components removed, voxels removed}).  A component of class k in 1 .. K - 1 with fewer than
    min_size[k] voxels becomes 0; exactly min_size[k] voxels stay."""
    cm = np.asarray(cm)
    thr = _thresholds(min_size, K)
    assert len(thr) == K
    out = cm.copy()
    stats = np.zeros((K, 2), np.int32)
    st = structure(cm.ndim, connectivity)
    for k in range(1, K):
        lab, n = ndimage.label(cm == k, st)
        if n == 0:
            continue
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        small = sizes < thr[k]
        small[0] = False
        out[small[lab]] = 0
        stats[k] = (int(small.sum()), int(sizes[small].sum()))
    return out, stats


def border_mask(shape):
    b = np.zeros(shape, bool)
    for ax in range(len(shape)):
        idx = [slice(None)] * len(shape)
        for edge in (0, shape[ax] - 1):
            idx[ax] = edge
            b[tuple(idx)] = True
    return b


def fill_holes(cm, K, connectivity=1):
    """-> (out, stats (K, 2) int32): row k >= 1 = {cavities filled with k, voxels filled}, row 0 = {cavities left because they touch
    two or more classes of 1 .. K - 1 (and nothing outside [0, K)), their voxels}."""
    cm = np.asarray(cm)
    out = cm.copy()
    stats = np.zeros((K, 2), np.int32)
    st = structure(cm.ndim, connectivity)
    lab, n = ndimage.label(cm == 0, st)
    on_border = np.zeros(n + 1, bool)
    on_border[np.unique(lab[border_mask(cm.shape)])] = True
    for j, box in enumerate(ndimage.find_objects(lab), start=1):
        if on_border[j]:
            continue
        # a cavity reaches no border, so its bounding box can grow by one voxel on every side
        grown = tuple(slice(s.start - 1, s.stop + 1) for s in box)
        comp = lab[grown] == j
        ring = ndimage.binary_dilation(comp, st) & ~comp
        contacts = np.unique(cm[grown][ring])
        assert contacts.size and (contacts != 0).all()
        if ((contacts < 1) | (contacts >= K)).any():
            continue
        size = int(comp.sum())
        if contacts.size == 1:
            k = int(contacts[0])
            out[grown][comp] = k
            stats[k] += (1, size)
        else:
            stats[0] += (1, size)
    return out, stats


def chain(cm, K, min_size, connectivity, keep_largest, fill_connectivity):
    """threshold -> keep-largest -> fill on one item, the order of the driver; keep_largest: a function (cm, K, connectivity) ->
    (out, stats) or None."""
    out, _ = remove_small(cm, K, min_size, connectivity)
    if keep_largest is not None:
        out, _ = keep_largest(out, K, connectivity)
    return fill_holes(out, K, fill_connectivity)[0]


# ---------------------------------------------------------------- inputs
def random_map(shape, K, seed, density=0.6, block=6):
    """A class map whose foreground class is constant on blocks of `block` voxels per axis (drawn from 1 .. K - 1, so that class
    K - 1 occurs whatever K), with value-0 voxels punched in at rate 1 - density: cavities inside a block have one contact class,
    cavities across a block boundary several, and specks of one class sit inside another where a block is a voxel wide."""
    rng = np.random.RandomState(seed)
    shape = tuple(shape)
    if K == 1:
        return (rng.rand(*shape) < 0.5).astype(np.int64) * 3                # no foreground class: every non-zero value is outside [0, K)
    coarse = tuple(-(-s // block) for s in shape)
    classes = rng.randint(1, K, size=coarse)
    classes.flat[0] = K - 1
    cm = classes
    for ax, s in enumerate(shape):
        cm = np.repeat(cm, block, axis=ax)
    cm = cm[tuple(slice(0, s) for s in shape)].astype(np.int64)
    speck = rng.rand(*shape) < 0.04                                      # single voxels of another class
    cm[speck] = rng.randint(1, K, size=int(speck.sum()))
    cm[rng.rand(*shape) >= density] = 0
    return cm


# ---------------------------------------------------------------- hand-drawn cases (2-D, K = 3 unless said)
def _parse(rows):
    return np.array([[int(ch) if ch != '.' else 0 for ch in r] for r in rows], np.int64)


def hand_drawn():
    """name -> dict(cm, K, ch, filled = {(y, x): class} of the voxels that change, stats row sums to check by eye)."""
    cases = {}
    ring = _parse(['.......',
                   '.11111.',
                   '.1...1.',
                   '.1...1.',
                   '.11111.',
                   '.......'])
    inner = {(y, x): 1 for y in (2, 3) for x in (2, 3, 4)}
    cases['ring'] = dict(cm=ring, K=3, ch=1, filled=inner, mixed=0)
    cases['ring ch2'] = dict(cm=ring, K=3, ch=2, filled=inner, mixed=0)
    leak = ring.copy()
    leak[1, 1] = 0                                                       # open at one diagonal: (2, 2) and (0, 0) .. (1, 1) touch by a corner
    cases['diagonal opening ch1'] = dict(cm=leak, K=3, ch=1, filled=inner, mixed=0)
    cases['diagonal opening ch2'] = dict(cm=leak, K=3, ch=2, filled={}, mixed=0)
    nested = _parse(['.........',
                     '.1111111.',
                     '.1.....1.',
                     '.1.222.1.',
                     '.1.2.2.1.',
                     '.1.222.1.',
                     '.1.....1.',
                     '.1111111.',
                     '.........'])
    cases['nested rings'] = dict(cm=nested, K=3, ch=1, filled={(4, 4): 2}, mixed=1)     # the moat between the rings touches 1 and 2
    corner = _parse(['.11111',
                     '1....1',
                     '1....1',
                     '111111'])
    room = {(y, x): 1 for y in (1, 2) for x in (1, 2, 3, 4)}
    cases['corner pixel ch1'] = dict(cm=corner, K=3, ch=1, filled=room, mixed=0)       # (0, 0) is a component of its own
    cases['corner pixel ch2'] = dict(cm=corner, K=3, ch=2, filled={}, mixed=0)         # (1, 1) - (0, 0): the region reaches the border there
    two = _parse(['......',
                  '.1122.',
                  '.1..2.',
                  '.1122.',
                  '......'])
    cases['two-class rim'] = dict(cm=two, K=3, ch=1, filled={}, mixed=1)
    out_of_range = _parse(['.....',
                           '.111.',
                           '.1.1.',
                           '.191.',
                           '.....'])
    cases['rim with a value outside [0, K)'] = dict(cm=out_of_range, K=3, ch=1, filled={}, mixed=0)
    return cases


def size_case(min_size=5):
    """A map with a component of exactly min_size pixels (stays) and one of min_size - 1 (goes), classes 1 and 2, and what is left."""
    cm = np.zeros((6, 2 * min_size + 3), np.int64)
    cm[1, 1:1 + min_size] = 1
    cm[3, 1:min_size] = 1
    cm[1, min_size + 2:2 * min_size + 2] = 2
    cm[4, min_size + 2:2 * min_size + 1] = 2
    want = cm.copy()
    want[3, 1:min_size] = 0
    want[4, min_size + 2:2 * min_size + 1] = 0
    return cm, want
