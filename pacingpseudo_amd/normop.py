"""The BatchNorm / GroupNorm + LeakyReLU side of one conv layer: the one object per layer and plan that makes its launches.

The counterpart of convop.py.  `NormOp` holds what is fixed for the plan and turns "this form, these operands" into the C-ABI
call(s) of that form; every launch goes through the plan's entry-point table K, looked up at call time.  What differs from call
to call -- training, synchronised BatchNorm, the engine's switches -- arrives as arguments.  Streams, events, the choice of
workspace and the calls into ConvOp stay in the engine.  `ws` arguments are (pointer, bytes) of the workspace of the stream `st`.
"""
from __future__ import annotations


class NormOp:
    """One layer's normalisation in one plan.  coef: its rows [mean, invstd, scale, shift] per statistics group (GroupNorm: per
    image, + xbar); z: the layer's own buffer for the pre-norm convolution output or None; lazy: the output stays lazy in train-
    mode BatchNorm; sums: per-channel sums of the split (synchronised) BatchNorm calls, [0] forward, [1] backward local, [2]
    backward global; zfull / dzfull: full-resolution z and zero-stuffed dz of a stride-2 layer; amax: the ConvOp's max |dz| cell.
    goff / boff: byte offsets added to the addresses of gamma / beta in the FORWARD calls -- 0: the live parameters; a teacher plan:
    the distance to the optimizer's shadow slab.  Running statistics are always the module's own."""
    __slots__ = ('K', 'C', 'gn', 'bn', 'slope', 'eps', 'mom', 'rows', 'xbar', 'z', 'lazy', 'sums', 'zfull', 'dzfull', 'am', 'goff', 'boff')

    def __init__(self, K, L, slope, eps, mom, coef, z, lazy, sums, zfull, dzfull, amax, goff=0, boff=0):
        self.K, self.C, self.gn, self.bn, self.slope = K, L.cout, L.gn, L.bn, slope
        self.goff, self.boff = goff, boff
        self.eps, self.mom = float(L.bn.eps) if L.gn else eps, mom
        self.rows = tuple(coef[i].data_ptr() for i in range(4))     # mean, invstd, scale, shift
        self.xbar = coef[4].data_ptr() if L.gn else None
        self.z, self.lazy, self.sums, self.zfull, self.dzfull = z, lazy, sums, zfull, dzfull
        self.am = amax.data_ptr() if amax is not None else None     # split-fp16 consumers scale dz by a power of two from max |dz|

    def z_dest(self, y, lazy):
        """(pointer, ld) of the pre-norm convolution output: in the buffer of the output y when that is lazy, else in the layer's
        own z buffer (a null pointer where it has none: the eval-mode epilogue of a lazy layer never stores z)."""
        return (y.ptr, y.ld) if lazy else (self.z.data_ptr() if self.z is not None else None, self.C)

    def params(self):
        bn = self.bn
        return bn.weight.data_ptr() + self.goff, bn.bias.data_ptr() + self.boff, bn.running_mean.data_ptr(), bn.running_var.data_ptr()

    def eval_coeffs(self, groups, st):
        self.K.pp_bn_eval_coeffs(self.C, groups, self.eps, *self.params(), *self.rows, st)

    def fwd(self, zptr, zld, y, groups, training, lazy, stats, sync, comm, world, pool_out, ws, st):
        """The layer's coefficient rows from z, then y = lrelu(z * scale + shift).  stats: (pointer, rows per group) of the
        per-block (sum, sum of squares) a fused convolution epilogue left, else None.  sync: statistics of the WHOLE batch of
        `world` ranks (models/unet.py:189) -- the local sums are taken in ONE row per group and all-reduced by `comm`.  lazy: no
        apply pass; the (scale, shift, slope) rows of y are written and y becomes a lazy tensor.  pool_out: the 2x2 max-pooled
        copy of y from the apply pass; returns whether it was written."""
        K, C, (mean, invstd, scale, shift) = self.K, self.C, self.rows
        if self.zfull is not None:      # stride 2: z = the stride-1 convolution output sampled at the even pixels (pp_spatial.hip)
            K.pp_stride2_gather(self.zfull.data_ptr(), C, zptr, C, C, y.N, y.H, y.W, st)
        n = ppg = (y.N // groups) * y.H * y.W
        if self.gn:                     # the same in train and eval mode: one coefficient row per image
            groups, ppg, gn = y.N, y.H * y.W, self.bn
            K.pp_gn_stats(zptr, zld, C, ppg, groups, gn.num_groups, self.eps, gn.weight.data_ptr() + self.goff, gn.bias.data_ptr() + self.boff,
                          mean, invstd, self.xbar, scale, shift, *ws, st)
        else:
            if sync:
                sums = self.sums[0]
                K.pp_bn_stats_sums(zptr, zld, C, ppg, groups, sums.data_ptr(), *ws, st)
                comm.allreduce_sums(sums)
                stats, n = (sums.data_ptr(), 1), ppg * world
            a = (C, n, groups, self.eps, self.mom, *self.params(), self.bn.num_batches_tracked.data_ptr(), *self.rows)
            if stats is None and not training:
                self.eval_coeffs(groups, st)
            elif stats is None:
                assert not lazy
                K.pp_bn_train_stats(zptr, zld, *a, *ws, st)
            elif lazy:
                K.pp_bn_train_finalize_lazy(*stats, *a, y.cptr, y.ld, self.slope, st)
                y.flag[0] = True
            else:
                K.pp_bn_train_finalize(*stats, *a, st)
        if lazy:
            return False
        if pool_out is not None:
            K.pp_bn_lrelu_fwd_pool(zptr, zld, scale, shift, y.ptr, y.ld, pool_out.ptr, pool_out.ld, C, y.N, y.H, y.W, groups,
                                   self.slope, st)
            return True
        K.pp_bn_lrelu_fwd(zptr, zld, scale, shift, y.ptr, y.ld, C, ppg, groups, self.slope, st)
        return False

    def bwd(self, dy, y, lazy, groups, pg, dz, pool, training, eval_fused, sync, comm, world, ws, st):
        """dz = gradient wrt the convolution output from dy, the gradient wrt the layer output y (lazy: y's buffer holds z).
        pg: pointers of the (norm weight, norm bias, conv bias) gradients.  pool: gradient of the 2x2-max-pooled copy of y, added
        to each window's winner.  eval_fused: the forward stored y only (eval-mode BatchNorm in the conv epilogue); sync: train-
        mode statistics over `world` ranks, their sums all-reduced by `comm` between the two launches.  Returns the pointer the
        convolution's gradients read: dz, or -- stride 2 -- dz scattered to the even pixels of dzfull."""
        K, C, (mean, invstd, scale, shift) = self.K, self.C, self.rows
        ppg = (y.N // groups) * y.H * y.W
        d = (dy.ptr, dy.ld) if pool is None else (dy.ptr, dy.ld, pool.ptr, pool.ld)
        zc = (*self.z_dest(y, lazy), scale, shift, mean, invstd)
        g = (dz, C, *pg, 0, C)
        gamma, tr = self.bn.weight.data_ptr(), 1 if training else 0
        tail = (self.slope, *ws, self.am, st)
        if self.gn:         # statistics of this forward per (image, group), whatever `training` and `sync` say
            fn, px = (K.pp_gn_lrelu_bwd, (y.H * y.W, y.N)) if pool is None else (K.pp_gn_lrelu_bwd_pool, (y.N, y.H, y.W))
            fn(*d, *zc, self.xbar, gamma, *g, *px, self.bn.num_groups, *tail)
        elif eval_fused:    # one pass over dy and y
            a = (*d, y.ptr, y.ld, scale, gamma, self.bn.bias.data_ptr(), *g)
            if pool is not None:
                K.pp_bn_lrelu_bwd_eval_pool(*a, y.N, y.H, y.W, *tail)
            else:
                K.pp_bn_lrelu_bwd_eval(*a, ppg * groups, *tail)
        elif pool is not None:
            K.pp_bn_lrelu_bwd_pool(*d, *zc, gamma, tr, *g, y.N, y.H, y.W, groups, *tail)
        elif sync:
            loc, glob = self.sums[1], self.sums[2]
            K.pp_bn_lrelu_bwd_sums(*d, *zc, C, ppg, groups, self.slope, loc.data_ptr(), *ws, st)
            glob.copy_(loc)
            comm.allreduce_sums(glob)
            K.pp_bn_lrelu_bwd_apply(*d, *zc, gamma, 1, loc.data_ptr(), glob.data_ptr(), ppg * world, *g, ppg, groups, *tail)
        elif self.am is not None:
            K.pp_bn_lrelu_bwd_amax(*d, *zc, gamma, tr, *g, ppg, groups, *tail)
        else:
            K.pp_bn_lrelu_bwd(*d, *zc, gamma, tr, *g, ppg, groups, self.slope, *ws, st)
        if self.dzfull is None:
            return dz
        K.pp_stride2_scatter(dz, C, self.dzfull.data_ptr(), C, C, y.N, y.H, y.W, st)
        return self.dzfull.data_ptr()

    def bwd_wgrad_c1(self, dy, y, lazy, x, groups, gw, pg, training, eval_fused, ws, st):
        """The first layer (one input channel, no data gradient): dz is formed and consumed by the weight gradient gw in one
        pass, never written."""
        _, _, scale, shift = self.rows
        ppg = (y.N // groups) * y.H * y.W
        xg = (x.ptr, x.ld, x.H, x.W, gw, 0, *pg, 0, self.C)
        if eval_fused:
            self.K.pp_bn_lrelu_bwd_eval_wgrad_c1(dy.ptr, dy.ld, y.ptr, y.ld, scale, self.bn.weight.data_ptr(),
                                                 self.bn.bias.data_ptr(), *xg, ppg * groups, self.slope, *ws, st)
        else:
            self.K.pp_bn_lrelu_bwd_wgrad_c1(dy.ptr, dy.ld, *self.z_dest(y, lazy), scale, shift, *self.rows[:2],
                                            self.bn.weight.data_ptr(), 1 if training else 0, *xg, ppg, groups, self.slope, *ws, st)
