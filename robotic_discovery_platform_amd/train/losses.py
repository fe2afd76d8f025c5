"""K-class training losses in plain torch: class-weighted softmax CE plus a soft Dice term.

``ce_dice_reference`` is the eager trainer's loss for ``"ce_dice"`` and for weighted ``"ce"``, and the
oracle of the native head's extended mode (csrc/head_multi.hip). With logits ``x[p][k]``,
``s = softmax(x[p])``, labels ``t[p]`` and a pixel *kept* iff ``t[p] < K`` (255 and K..254 are ignored):

    W    = sum_kept w[t_p]
    CE   = sum_kept w[t_p] * (logsumexp(x_p) - x_p[t_p]) / W          (0 if W == 0)
    I_k  = sum_kept s_pk [t_p == k],  P_k = sum_kept s_pk,  T_k = sum_kept [t_p == k]
    Dice = 1 - (1/K) sum_k (2 I_k + eps) / (P_k + T_k + eps)          (all K classes)
    L    = CE + dice_weight * Dice

The sums run over the whole batch. The class weights act on CE only. CE is
``F.cross_entropy(x, t, weight=w, ignore_index=255)``, except that with nothing kept (or W == 0) the
loss is 0 with zero gradients where torch gives NaN.
"""
from typing import Optional, Sequence, Tuple

import torch


def check_class_weights(class_weights, n_classes: int) -> Optional[Tuple[float, ...]]:
    """``class_weights`` (None, or a sequence of K numbers) -> a tuple of K finite, non-negative floats
    with at least one positive, or None. Anything else raises ``ValueError``."""
    if class_weights is None:
        return None
    if isinstance(class_weights, torch.Tensor):
        class_weights = class_weights.detach().cpu().tolist()
    try:
        vals = tuple(float(v) for v in class_weights)
    except (TypeError, ValueError) as e:
        raise ValueError(f"class_weights must be a sequence of {n_classes} numbers, got {class_weights!r}") from e
    if len(vals) != n_classes:
        raise ValueError(f"class_weights must list {n_classes} values (one per class), got {len(vals)}")
    if any(v != v or v in (float("inf"), float("-inf")) or v < 0 for v in vals):
        raise ValueError(f"class_weights must be finite and >= 0, got {vals}")
    if not any(v > 0 for v in vals):
        raise ValueError("class_weights must have at least one positive value")
    return vals


def parse_class_weights(text) -> Optional[Tuple[float, ...]]:
    """``"1,4,4"`` (or a sequence) -> (1.0, 4.0, 4.0); empty -> None (the format of ``mask_values``)."""
    if text is None or (isinstance(text, str) and not text.strip()):
        return None
    vals = tuple(float(v) for v in (text.split(",") if isinstance(text, str) else text))
    return vals or None


def ce_dice_reference(logits: torch.Tensor, labels: torch.Tensor, class_weights: Optional[Sequence[float]] = None,
                      dice_weight: float = 0.0, eps: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``logits`` [N,K,H,W] (any float dtype: the loss is computed in it), ``labels`` [N,H,W] or
    [N,1,H,W] integer class ids. Returns ``(L, CE)``, both differentiable scalars."""
    K = logits.shape[1]
    t = labels.long()
    if t.dim() == 4:
        t = t.squeeze(1)
    x = logits.permute(0, 2, 3, 1).reshape(-1, K)
    t = t.reshape(-1)
    kept = (t >= 0) & (t < K)
    x, t = x[kept], t[kept]
    if class_weights is None:
        w = torch.ones(K, dtype=x.dtype, device=x.device)
    else:
        w = torch.as_tensor(class_weights, dtype=x.dtype, device=x.device)
    logp = torch.log_softmax(x, dim=1)
    wt = w[t]
    W = wt.sum()
    ce_sum = -(wt * logp.gather(1, t[:, None]).squeeze(1)).sum()
    ce = torch.where(W > 0, ce_sum / torch.where(W > 0, W, torch.ones_like(W)), torch.zeros_like(W))  # no sync
    s = logp.exp()
    onehot = torch.nn.functional.one_hot(t, K).to(x.dtype)
    inter = (s * onehot).sum(0)
    dice = 1.0 - ((2.0 * inter + eps) / (s.sum(0) + onehot.sum(0) + eps)).mean()
    return ce + dice_weight * dice, ce
