"""Helper, not a test: torch restatement of the speaker encoder's loss (Speaker_Embedding/Modules.py:39-98) with both
Loss_Calc_Methods, in the dtype of its input (float64 as the reference of the kernels, float32 to measure the formula's own rounding)."""
import torch


def ge2e_logits(x_last, P, w, b):
    """Embedding_Generate + the similarities: x_last [S*P, D], speaker-major -> (within [S, P], between [S, P, S - 1])."""
    e = x_last * torch.rsqrt(torch.clamp((x_last * x_last).sum(dim=1, keepdim=True), min=1e-12))
    N, D = e.shape
    S = N // P
    r = e.reshape(S, P, D)
    cw = (r.sum(dim=1, keepdim=True) - r) / (P - 1)
    cb = r.mean(dim=1)
    cos = lambda a, c: (a * c).sum(-1) / (torch.sqrt((a ** 2).sum(-1)) * torch.sqrt((c ** 2).sum(-1)))
    within = w * cos(r, cw) - b
    tx, ty = e[:, None, :], cb[None, :, :]
    cos2 = (ty * tx).sum(2) / (torch.sqrt((ty ** 2).sum(2)) * torch.sqrt((tx ** 2).sum(2)) + 1e-8)
    between = (w * cos2 - b).reshape(S, P, S)
    keep = ~torch.eye(S, dtype=torch.bool)[:, None, :].expand(S, P, S)
    return within, between[keep].reshape(S, P, S - 1)


def ge2e_softmax(x_last, P, w, b):
    within, between = ge2e_logits(x_last, P, w, b)
    return -(torch.log_softmax(torch.cat([within[..., None], between], dim=-1), dim=-1)[..., 0]).mean()


def ge2e_contrast(x_last, P, w, b):
    """Modules.py:94: reduce_sum(1 - sigmoid(within) + reduce_max(between, -1))."""
    within, between = ge2e_logits(x_last, P, w, b)
    return (1 - torch.sigmoid(within) + between.max(dim=-1).values).sum()


def between_gap(x_last, P, w, b):
    """Smallest difference between a row's two largest between-speaker logits (1-D when there is one other speaker: +inf)."""
    _, between = ge2e_logits(x_last, P, w, b)
    if between.shape[-1] < 2:
        return float("inf")
    top = between.detach().topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())
