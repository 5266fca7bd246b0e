"""Pure-torch restatement of the masked-LM loss (float64), the reference of tests/test_mlm_eval.py and tests/test_gpu_mlm_loss.py.

    nll[b, p] = logsumexp_v(logits[b, p, :]) - logits[b, p, label]       over all 8 (padded-vocabulary) logits
    ignored:    label == ignore_index or label < 0 (nll 0, no contribution)
    unweighted: loss = mean of nll over the labelled positions of the batch
    weighted:   loss = sum(w nll) / sum(w) with w zeroed at ignored positions        (the public Caduceus model code, recalled)
Both are nan for a batch without labelled positions / without weight (0 / 0), as F.cross_entropy's mean is."""
import numpy as np
import torch


def labelled_mask(labels, ignore_index=-100):
    labels = torch.as_tensor(labels).long()
    return ~((labels == ignore_index) | (labels < 0))


def token_nll(logits, labels, ignore_index=-100):
    """float64 [B, L]: per-token cross entropy, 0 at ignored positions."""
    lg = torch.as_tensor(logits).double()
    labels = torch.as_tensor(labels).long()
    m = labelled_mask(labels, ignore_index)
    lsm = torch.log_softmax(lg, dim=-1)
    nll = -lsm.gather(-1, labels.clamp(0, lg.shape[-1] - 1).unsqueeze(-1)).squeeze(-1)
    return torch.where(m, nll, torch.zeros_like(nll))


def window_sums(logits, labels, weights=None, ignore_index=-100):
    """float64 [B, 4]: sum w nll, sum w, labelled positions, labelled positions whose arg-max logit (first on ties) is the label."""
    lg = torch.as_tensor(logits).double()
    labels = torch.as_tensor(labels).long()
    m = labelled_mask(labels, ignore_index)
    nll = token_nll(lg, labels, ignore_index)
    w = torch.ones_like(nll) if weights is None else torch.as_tensor(weights).double()
    w = torch.where(m, w, torch.zeros_like(w))
    hit = (lg.argmax(-1) == labels) & m
    return torch.stack([(w * nll).sum(1), w.sum(1), m.double().sum(1), hit.double().sum(1)], dim=1)


def loss(logits, labels, weights=None, ignore_index=-100):
    """float64 scalar: the batch loss by the formula that applies (mean over labelled positions / weighted mean)."""
    nll = token_nll(logits, labels, ignore_index)
    m = labelled_mask(labels, ignore_index)
    if weights is None:
        return nll[m].mean() if m.any() else torch.tensor(float("nan"), dtype=torch.float64)
    w = torch.where(m, torch.as_tensor(weights).double(), torch.zeros_like(nll))
    return (w * nll).sum() / w.sum()


def trainer_eval_loss(logits, labels, weights, batch_size, ignore_index=-100):
    """Trainer.evaluation_loop's eval_loss: the loss of every batch of `batch_size` consecutive windows repeated once per window,
    concatenated, mean."""
    n = len(labels)
    rep = []
    for b0 in range(0, n, batch_size):
        b1 = min(b0 + batch_size, n)
        l = loss(logits[b0:b1], labels[b0:b1], None if weights is None else weights[b0:b1], ignore_index)
        rep += [float(l)] * (b1 - b0)
    return float(np.mean(rep)) if rep else float("nan")
