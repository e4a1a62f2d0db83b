"""Label losses (cs/losses.py), selected by name with --label_loss (cs/train.py:67).  CrossEntropyLoss, the default, is
evc_ce_loss; the seven other scalar losses of the reference - CrossEntropyLossWithSparsity, CrossEntropyLossTop50,
CrossEntropyLossClassImbalance, CrossEntropyLossPositives, NewLoss, HingeLoss, SoftmaxLoss - are the kinds of evc_label_loss
(value and dL/dpredictions in one pass; definitions in include/evc.h and DESIGN.md 7.7) and train, validate and fine-tune like the
default.  PWELoss exists by name and refuses to compute: the reference's own graph cannot train on it (see the class)."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops


class BaseLoss(object):
    """cs/losses.py:8-25."""

    kind = None          # ops.LOSS_* of the evc_label_loss kinds; None: CrossEntropyLoss (evc_ce_loss) and BaseLoss itself

    def calculate_loss(self, unused_predictions, unused_labels, **unused_params):
        raise NotImplementedError()

    def check(self, vocab_size):
        """What this loss refuses for ``vocab_size`` classes, raised on the host before anything touches the device."""

    def fused(self, pred, labels_u8, loss, dpred=None, grad_scale=1.0, accumulate_grad=False):
        """The graphs' call: loss[0] += mean_b row loss, dpred (= | +=) grad_scale * d(sum_b row loss)/dpred (ops.ce_loss's contract)."""
        raise NotImplementedError()


class CrossEntropyLoss(BaseLoss):
    """mean_b sum_c -(y log(p+1e-5) + (1-y) log(1-p+1e-5))   (cs/losses.py:90-97).

    Returns a 0-d device tensor.  ``grad_out`` (optional [B,V] f32) receives
    dLoss/dpredictions in the same pass (the training graph feeds it straight to
    the model's backward instead of building an autograd tape)."""

    def calculate_loss(self, predictions, labels, grad_out=None, **unused_params):
        B, V = predictions.shape
        lab = labels if labels.dtype == torch.uint8 else labels.to(torch.uint8)
        loss = torch.zeros(1, dtype=torch.float32, device=predictions.device)
        ops.ce_loss(predictions, lab.contiguous(), loss, grad_out, grad_scale=1.0 / B)
        return loss[0]

    def fused(self, pred, labels_u8, loss, dpred=None, grad_scale=1.0, accumulate_grad=False):
        ops.ce_loss(pred, labels_u8, loss, dpred, grad_scale=grad_scale, accumulate_grad=accumulate_grad)


class _LabelLoss(BaseLoss):
    """A kind of evc_label_loss: ``calculate_loss`` has the contract of CrossEntropyLoss.calculate_loss."""

    def class_weights(self, vocab_size, device):
        return None

    def check(self, vocab_size):
        if vocab_size > ops.LABEL_LOSS_MAX_V:
            raise ValueError("--label_loss %s: %d classes (at most %d)" % (type(self).__name__, vocab_size, ops.LABEL_LOSS_MAX_V))

    def fused(self, pred, labels_u8, loss, dpred=None, grad_scale=1.0, accumulate_grad=False):
        ops.label_loss(self.kind, pred, labels_u8, loss, dpred, grad_scale=grad_scale, accumulate_grad=accumulate_grad,
                       class_weights=self.class_weights(pred.shape[1], pred.device))

    def calculate_loss(self, predictions, labels, grad_out=None, **unused_params):
        B, V = predictions.shape
        self.check(V)
        lab = labels if labels.dtype == torch.uint8 else labels.to(torch.uint8)
        loss = torch.zeros(1, dtype=torch.float32, device=predictions.device)
        self.fused(predictions, lab.contiguous(), loss, grad_out, grad_scale=1.0 / B)
        return loss[0]


class CrossEntropyLossWithSparsity(_LabelLoss):
    """Cross entropy + 0.1 mean_b sum_c p   (cs/losses.py:28-41)."""
    kind = ops.LOSS_WITH_SPARSITY


class CrossEntropyLossTop50(_LabelLoss):
    """(4716/50) x the cross entropy of the classes whose prediction is at least the row's 50th largest (ties kept; the mask carries no
    gradient; cs/losses.py:43-60).  Needs 50 classes, as tf.nn.top_k does."""
    kind = ops.LOSS_TOP50

    def check(self, vocab_size):
        if vocab_size < 50:
            raise ValueError("--label_loss CrossEntropyLossTop50 needs at least 50 classes (got %d): it takes each row's 50th largest "
                             "prediction" % vocab_size)
        super().check(vocab_size)


TOTAL_LABEL_COUNT = 4906660.0 + 1401828.0     # cs/losses.py:109: the training + validation videos the counts were taken over


def load_class_weights(path, vocab_size):
    """--label_loss_counts_file: one integer per line, ``vocab_size`` lines -> w_c = float32(1 / sqrt(count_c / TOTAL_LABEL_COUNT)),
    computed in float64 as the reference does (cs/losses.py:107-114).  Every defect is a ValueError that names the flag."""
    what = "--label_loss_counts_file %s" % path
    if not os.path.isfile(path):
        raise ValueError("%s: no such file (CrossEntropyLossClassImbalance reads one class count per line from it)" % what)
    with open(path, "r") as f:
        lines = [ln.strip() for ln in f.readlines()]
    while lines and not lines[-1]:
        lines.pop()
    try:
        counts = np.array([int(ln) for ln in lines], dtype=np.int64)
    except ValueError as e:
        raise ValueError("%s: not one integer per line (%s)" % (what, e))
    if counts.size != vocab_size:
        raise ValueError("%s: %d lines for %d classes" % (what, counts.size, vocab_size))
    if (counts <= 0).any():
        raise ValueError("%s: the count of class %d is %d (every count must be positive)" % (what, int(np.argmax(counts <= 0)),
                                                                                          int(counts[np.argmax(counts <= 0)])))
    return (1.0 / np.sqrt(counts.astype(np.float64) / TOTAL_LABEL_COUNT)).astype(np.float32)


class CrossEntropyLossClassImbalance(_LabelLoss):
    """Cross entropy with the positive term of class c weighted by w_c = 1 / sqrt(count_c / 6308488) (cs/losses.py:99-119); the counts
    come from --label_loss_counts_file (default counts_tv, the name the reference opens in the working directory), or ``weights``."""
    kind = ops.LOSS_CLASS_IMBALANCE

    def __init__(self, counts_file=None, weights=None):
        self.counts_file = counts_file
        self._host = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        self._dev = {}

    def host_weights(self, vocab_size):
        if self._host is None:
            from .flags import FLAGS
            self._host = load_class_weights(self.counts_file or FLAGS.label_loss_counts_file, vocab_size)
        if self._host.size != vocab_size:
            raise ValueError("--label_loss_counts_file: %d class weights for %d classes" % (self._host.size, vocab_size))
        return self._host

    def check(self, vocab_size):
        super().check(vocab_size)
        self.host_weights(vocab_size)

    def class_weights(self, vocab_size, device):
        key = (str(device), vocab_size)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.host_weights(vocab_size)).to(device)
        return self._dev[key]


class CrossEntropyLossPositives(_LabelLoss):
    """The positive half of the cross entropy alone: -y log(p + eps)   (cs/losses.py:121-131)."""
    kind = ops.LOSS_POSITIVES


class NewLoss(_LabelLoss):
    """Cross entropy of the "bad" elements only: positives below 0.9 and negatives above max(min positive of the BATCH - 0.1, 0.1)
    (cs/losses.py:133-151).  The batch is the [B, V] matrix of the call: per rank under data parallelism, as the reference computes its
    label loss per tower."""
    kind = ops.LOSS_NEW


class HingeLoss(_LabelLoss):
    """mean_b sum_c max(0, 1 - (2y - 1) p), subgradient 0 at the tie   (cs/losses.py:153-169, b = 1)."""
    kind = ops.LOSS_HINGE


class SoftmaxLoss(_LabelLoss):
    """mean_b -sum_c yhat_c log softmax(p)_c with yhat = y / max(sum y, 10e-8)   (cs/losses.py:172-196)."""
    kind = ops.LOSS_SOFTMAX


class PWELoss(BaseLoss):
    """cs/losses.py:62-84: not built.  The reference's class reshapes to a hard-wired [128, 4716] and returns a [4716, 4716] matrix
    instead of a scalar, so the reference's own graph cannot train on it."""

    MESSAGE = ("PWELoss is not built: cs/losses.py:62-84 reshapes to a hard-wired [128, 4716] and returns a [4716, 4716] matrix, not a "
               "scalar - the reference's own graph cannot train on it")

    def check(self, vocab_size):
        raise NotImplementedError(self.MESSAGE)

    def fused(self, *unused_args, **unused_params):
        raise NotImplementedError(self.MESSAGE)

    def calculate_loss(self, unused_predictions, unused_labels, **unused_params):
        raise NotImplementedError(self.MESSAGE)


def resolve(label_loss):
    """None (CrossEntropyLoss), a class name of this module or a BaseLoss instance -> the instance."""
    if label_loss is None:
        return CrossEntropyLoss()
    if isinstance(label_loss, BaseLoss):
        return label_loss
    cls = globals().get(label_loss) if isinstance(label_loss, str) else None
    if not (isinstance(cls, type) and issubclass(cls, BaseLoss)) or cls in (BaseLoss, _LabelLoss):
        raise ValueError("label_loss %r: a losses.BaseLoss instance or the name of one of its classes" % (label_loss,))
    return cls()


def is_default(label_loss_fn):
    return type(label_loss_fn) is CrossEntropyLoss
