"""Shared inputs of the confusion-matrix tests (CPU reference and GPU kernel)."""
import torch


def planted_case(K, M, seed=0, thr=0.0):
    """Logits on a quarter grid (ties are frequent) with planted exact ties -- two and three equal maxima
    and all-equal pixels -- and labels with ~10 % 255 and a few 200. K == 1: float targets, and logits
    exactly at ``thr``. Returns (logits [M*K] fp32, target [M])."""
    g = torch.Generator().manual_seed(1000 * K + seed)
    x = (torch.randint(-6, 7, (M, K), generator=g).float() / 4)
    if K == 1:
        x[::7, 0] = thr  # exactly at the threshold: not foreground (strict >)
        t = (torch.rand(M, generator=g) > 0.6).float()
        return x.reshape(-1).contiguous(), t
    x[0::11] = 0.75  # all equal -> class 0
    x[1::11, 0] = -5.0
    x[1::11, 1:] = 1.0  # every class but 0 ties -> class 1
    if K >= 3:
        x[2::11] = -2.0
        x[2::11, K - 2:] = 2.5  # the last two tie -> K - 2
        x[3::11] = -1.0
        x[3::11, [0, K // 2, K - 1]] = 1.5  # three equal maxima -> class 0
    t = torch.randint(0, K, (M,), generator=g, dtype=torch.int64)
    t[torch.rand(M, generator=g) < 0.1] = 255
    t[5::37] = 200
    return x.reshape(-1).contiguous(), t.to(torch.uint8)


def brute_force(x, t, K, thr):
    kc = max(K, 2)
    c = [0] * (kc * kc + 1)
    M = t.numel()
    xl, tl = x.view(M, K).tolist(), t.tolist()
    for p in range(M):
        if K == 1:
            c[(2 if tl[p] > 0.5 else 0) + (1 if xl[p][0] > thr else 0)] += 1
            continue
        if tl[p] >= K:
            c[kc * kc] += 1
            continue
        best = 0
        for k in range(1, K):
            if xl[p][k] > xl[p][best]:
                best = k
        c[int(tl[p]) * kc + best] += 1
    return torch.tensor(c, dtype=torch.int64)
