"""numpy fp64 definition of the test-time-augmentation views and their mean (the specification of utils/tta.py; the reference
project has no such mode).  op: bit 0 flips the last axis, bit 1 the second-to-last, bit 2 transposes them; the forward view
is transpose, flip H, flip W in that order, the inverse the same steps backwards."""
import numpy as np


def view(a, op):
    b = np.asarray(a)
    if op & 4:
        b = np.swapaxes(b, -1, -2)
    if op & 2:
        b = np.flip(b, -2)
    if op & 1:
        b = np.flip(b, -1)
    return b.copy()                                    # a fresh C-ordered array (a flipped axis of length 1 keeps its negative stride otherwise)


def inverse(a, op):
    b = np.asarray(a)
    if op & 1:
        b = np.flip(b, -1)
    if op & 2:
        b = np.flip(b, -2)
    if op & 4:
        b = np.swapaxes(b, -1, -2)
    return b.copy()


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def tta_mean(view_logits, ops):
    """view_logits[v]: (N, K, H', W') logits of view ops[v] -> (prob (N, K, H, W) float64, cls (N, H, W) = first-maximum arg-max)."""
    assert len(view_logits) == len(ops)
    acc = None
    for z, op in zip(view_logits, ops):
        p = inverse(softmax(z), op)
        acc = p if acc is None else acc + p
    prob = acc / len(ops)
    return prob, prob.argmax(1)
