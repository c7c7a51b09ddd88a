"""fp64 reference of ops.lora_apply and its error bound, over the very bf16
tensors the op gets (tests/test_lora_batched*.py)."""
import torch


def reference(y0, x, slots, rows):
    """(ref, bound): ref[t] = y0[t] + B_s (scale_s A_s x[t]) for s = slots[t]
    with rows[s] = (A, B, scale) or None, and elementwise
    2^-8 |ref| + 2^-8 sum_r |B[n, r]| |v[t, r]| + 1e-6: the output rounding and
    the bf16 rounding of v, each doubled."""
    ref = y0.double().cpu().clone()
    slack = torch.zeros_like(ref)
    slots = slots.cpu()
    for s, row in enumerate(rows):
        if s == 0 or row is None:
            continue
        A, B, scale = (w.double().cpu() if torch.is_tensor(w) else w for w in row)
        idx = (slots == s).nonzero(as_tuple=True)[0]
        v = scale * (x[idx.to(x.device)].double().cpu() @ A.T)
        ref[idx] += v @ B.T
        slack[idx] = v.abs() @ B.abs().T
    return ref, 2.0**-8 * ref.abs() + 2.0**-8 * slack + 1e-6
