"""Non-finite activations for the conv tests (tests/test_gpu_conv.py, tests/test_gpu_tile_paths.py): an
input with +-inf, NaN and a signalling NaN planted in it, and the comparison of an output's non-finite
pattern with a reference's."""
import torch


def nonfinite_input(N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:6]
    sig = torch.tensor([0x7F800001], dtype=torch.int32).view(torch.float32)  # signaling NaN, low payload only
    for v, i in zip((float("inf"), float("-inf"), float("nan"), float("inf"), sig.item(), float("-inf")), idx):
        flat[i] = v
    return x


def same_nonfinite(y, ref):
    return (torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(torch.isposinf(y), torch.isposinf(ref))
            and torch.equal(torch.isneginf(y), torch.isneginf(ref)))
