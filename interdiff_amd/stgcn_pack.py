"""Host side of the ST-GCN correction predictors (``objprojector.py``: SMPL markers, ``skeleton.py``: HO-GCN joints): the float32 arena
both kernels read.  Folded on the host in float64:
  * eval-mode BatchNorm into the preceding 1x1 convolution (tcn.0/tcn.1 and residual.0/residual.1);
  * the idx_pad frame repetition (future frames = last past frame) into ``dct_pad`` [n_pre, past_len];
  * DCT / IDCT matrices exactly as get_dct_matrix builds them (fp64, inverse by numpy) -> fp32.
The layout of a layer block is described once, in csrc/stgcn.h (``layer_params`` reads what ``pack_stgcn_layers`` writes).
"""
import numpy as np
import torch

STACKS = ('st_gcnns_relative', 'st_gcnns', 'st_gcnns_all')


def dct_matrices(N):
    k = np.arange(N)[:, None].astype(np.float64)
    i = np.arange(N)[None, :].astype(np.float64)
    w = np.full((N, 1), np.sqrt(2.0 / N))
    w[0, 0] = np.sqrt(1.0 / N)
    d = w * np.cos(np.pi * (i + 0.5) * k / N)
    return d, np.linalg.inv(d)


def to_f64(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def fold_bn(sd, conv, bn, eps=1e-5):
    W, b = to_f64(sd[conv + '.weight'])[:, :, 0, 0], to_f64(sd[conv + '.bias'])
    g, beta = to_f64(sd[bn + '.weight']), to_f64(sd[bn + '.bias'])
    mu, var = to_f64(sd[bn + '.running_mean']), to_f64(sd[bn + '.running_var'])
    s = g / np.sqrt(var + eps)
    return W * s[:, None], (b - mu) * s + beta


def _pad16(n):
    return -(-n // 16) * 16


class ArenaBuilder:
    """float32 pieces, each starting on a multiple of 16 floats (zero padded): the kernels' float4 loads stay aligned."""

    def __init__(self):
        self.parts, self.n = [], 0

    def add(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32).ravel()
        off, pad = self.n, (-a.size) % 16
        self.parts += [a, np.zeros(pad, np.float32)]
        self.n += a.size + pad
        return off

    def arena(self):
        return np.concatenate(self.parts)


def pack_dct(builder, T, n_pre, past_len):
    """-> offsets (dct_pad [n_pre, past_len], dct [n_pre, T], idct [T, n_pre])."""
    dct, idct = dct_matrices(T)
    d = dct[:n_pre]
    dpad = d[:, :past_len].copy()
    dpad[:, past_len - 1] = d[:, past_len - 1:].sum(axis=1)
    return builder.add(dpad), builder.add(d), builder.add(idct[:, :n_pre])


def pack_stgcn_layers(builder, sd, op, n_pre, vp):
    """The 12 layer blocks (csrc/stgcn.h) of the three stacks; fills ``op.layer / cin / cout``."""
    for li in range(12):
        p = '%s.%d' % (STACKS[li // 4], li % 4)
        Wt, bt = fold_bn(sd, p + '.tcn.0', p + '.tcn.1')
        Wr, br = fold_bn(sd, p + '.residual.0', p + '.residual.1')
        cout, cin = Wt.shape
        W, b = np.zeros((2, _pad16(cout), _pad16(cin))), np.zeros((2, _pad16(cout)))
        W[:, :cout, :cin], b[:, :cout] = (Wt, Wr), (bt, br)
        Tm = to_f64(sd[p + '.gcn.T']).ravel()
        blk = [Tm, np.zeros(_pad16(Tm.size) - Tm.size)]
        if li // 4 == 2:
            A = to_f64(sd[p + '.gcn.A'])                               # [n_pre, nodes, nodes] : y[w] = sum_v x[v] A[t][v][w]
            AT = np.zeros((n_pre, vp, vp))
            AT[:, :A.shape[2], :A.shape[1]] = A.transpose(0, 2, 1)     # [t][w][v], zero padded to vp x vp
            blk.append(AT.ravel())
        blk += [W[0].ravel(), b[0], W[1].ravel(), b[1], to_f64(sd[p + '.prelu.weight']).ravel()]
        op.layer[li] = builder.add(np.concatenate(blk))
        op.cout[li], op.cin[li] = cout, cin


def unpack_stgcn_layers(op, arena, n_pre, vp, nodes):
    """The 12 folded layers back out of a packed arena (float32), as dicts Tm, A (joint stack over ``nodes`` nodes), Wt, bt, Wr, br,
    prelu -- what a CPU restatement evaluates to check the packer."""
    out = []
    for li in range(12):
        v2, cin, cout = li // 4 == 2, op.cin[li], op.cout[li]
        cinp, coutp = _pad16(cin), _pad16(cout)
        o = [op.layer[li]]

        def take(n, *shape):
            o[0] += n
            return arena[o[0] - n:o[0]].reshape(shape or n)
        L = {}
        nT = (nodes if v2 else 1) * n_pre * n_pre
        L['Tm'] = take(_pad16(nT))[:nT].reshape((nodes, n_pre, n_pre) if v2 else (n_pre, n_pre))
        if v2:
            L['A'] = take(n_pre * vp * vp, n_pre, vp, vp)[:, :nodes, :nodes].transpose(0, 2, 1)
        L['Wt'], L['bt'] = take(coutp * cinp, coutp, cinp)[:cout, :cin], take(coutp)[:cout]
        L['Wr'], L['br'] = take(coutp * cinp, coutp, cinp)[:cout, :cin], take(coutp)[:cout]
        L['prelu'] = arena[o[0]]
        out.append(L)
    return out
