"""Long-double restatement of the classifier read-out (mpst_eval, mpst_classify, mpst_classify_batch): the overlaps of an MPS whose
label index sits on ANY site with a set of product states, and what summary.jl:4-136 derives from them - predictions, the MSE and
KLD of every series and their means, the accuracy and the confusion counts.

The overlaps come from oracle.ref_numpy.contract_mps on np.longdouble / np.clongdouble copies of the inputs (its einsum calls keep
that type for a label on any site); everything after them is computed in long double as well, so that the reference's own error
(1e-19 relative on x86, 4e-16 ... 1.1e-15 of the largest overlap for the float64 oracle, tests/test_readout_ref.py) lies far below
every bound a device result is held to."""
import numpy as np

from oracle import ref_numpy as R


def ragged_chain(dims, d, C, label_site, cx, rng, scale=None):
    """Gaussian site tensors (dims[j], d, dims[j + 1]) for the bond profile ``dims`` (dims[0] == dims[T] == 1), the label tensor
    (Dl, d, Dr, C) on ``label_site``; every site is scaled by 1 / sqrt(Dl d), which keeps the overlaps with unit product states of
    order 0.1.  ``scale``: per-site factors, exact powers of two, applied on top."""
    T = len(dims) - 1
    assert dims[0] == 1 and dims[T] == 1 and 0 <= label_site < T
    W = []
    for j in range(T):
        shape = (dims[j], d, dims[j + 1]) + ((C,) if j == label_site else ())
        t = rng.standard_normal(shape)
        if cx:
            t = t + 1j * rng.standard_normal(shape)
        t = t / np.sqrt(dims[j] * d)
        if scale is not None:
            m, _ = np.frexp(float(scale[j]))
            assert m == 0.5, "scale factors are powers of two"
            t = t * float(scale[j])
        W.append(t)
    return W


def wide(x):
    return np.asarray(x).astype(np.clongdouble if np.iscomplexobj(x) else np.longdouble)


def overlaps_ld(W, phi):
    """(N, C) overlaps in long double"""
    cx = np.iscomplexobj(phi) or any(np.iscomplexobj(t) for t in W)
    dt = np.clongdouble if cx else np.longdouble
    y = R.contract_mps([np.asarray(t).astype(dt) for t in W], np.asarray(phi).astype(dt))
    assert y.dtype == dt
    return y


def readout_from(y, labels):
    """What MSE_loss_acc_conf and classify make of the overlaps ``y`` (N, C), in y's precision."""
    labels = np.asarray(labels)
    N, C = y.shape
    rows = np.arange(N)
    mag = np.abs(y)
    pred = np.argmax(mag, axis=1)                                   # the first largest |y|
    onehot = np.zeros((N, C), dtype=mag.dtype)
    onehot[rows, labels] = 1
    mse = np.sum(np.abs(y - onehot) ** 2, axis=1) / 2
    kld = -np.log(mag[rows, labels] ** 2)
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (labels, pred), 1)                              # conf[truth][pred]
    if C > 1:
        top = np.sort(mag, axis=1)
        gap = (top[:, -1] - top[:, -2]) / top[:, -1]
    else:
        gap = np.ones(N, dtype=mag.dtype)
    return dict(y=y, pred=pred, mse=mse, kld=kld, mse_mean=mse.mean(), kld_mean=kld.mean(),
                acc=float(np.count_nonzero(pred == labels)) / N, conf=conf, gap=gap)


def readout_ref(W, phi, labels):
    return readout_from(overlaps_ld(W, phi), labels)
