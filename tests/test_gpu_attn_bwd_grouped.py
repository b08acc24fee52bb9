"""ar_attn_bwd_exact_grouped (csrc/ar_attn_exact.hip: the persistent key-side kernel that sums the query-head group) against autograd of
`F.scaled_dot_product_attention(q, repeat_kv(k), repeat_kv(v), attn_mask=<0 / 1 additive mask>)` on the GPU -- dq / dk / dv value for
value, as tests/test_gpu_attn_exact.py checks the per-head form (the call transformers' `sdpa_attention_forward` makes under the
reference's `block_forward`: auto_round/compressors/utils.py:109-172).  The shapes are the smallest that reach every branch of the
kernel; S <= 256 is left out at head size 128 (the library's bits are not restated there)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SCALE = 128 ** -0.5
# B, H, hk, S, D
REP4 = (1, 8, 2, 512, 128)            # 8 items: fewer than CUs
REP8 = (2, 8, 1, 384, 128)            # S % 256 == 128, three key blocks; groups of 8: all heads park, (j, j + 4) pairs summed first
REP1 = (1, 4, 4, 640, 128)            # no sum: the head's result written directly
REP2 = (3, 24, 12, 1152, 128)         # 324 items: more than the CUs and no multiple; several items and item boundaries per workgroup


def _ndiff(a, b):
    a, b = a.contiguous(), b.contiguous()
    return int((a.view(torch.int16) != b.view(torch.int16)).sum())


@functools.lru_cache(maxsize=None)
def _case(shape, head_scaled=False, std=SCALE, cancel=False):
    """operands, the first-party forward's results and torch's gradients for one shape: computed once, shared, never written to"""
    from auto_round_amd import ops

    B, H, hk, S, D = shape
    rep = H // hk
    scale = D ** -0.5 if D == 128 else 1.0
    torch.manual_seed(B * 1000 + S)
    dev = "cuda"
    qb = (torch.randn(B, S, H, D, device=dev) * std).to(torch.bfloat16)
    if cancel:           # groups of 8: head j + 4 asks what head j asks ...
        qg = qb.view(B, S, hk, rep, D)
        qg[:, :, :, 4:] = qg[:, :, :, :4]
    q = qb.transpose(1, 2)
    k = (torch.randn(B, S, hk, D, device=dev) * std).to(torch.bfloat16).transpose(1, 2)
    v = torch.randn(B, S, hk, D, device=dev).to(torch.bfloat16).transpose(1, 2)
    idx = torch.arange(S, device=dev)
    keep = (idx[None, :] <= idx[:, None]) & (idx[None, :] < S - 1)
    mask = keep.to(torch.bfloat16)[None, None].expand(B, 1, S, S).contiguous()
    st = ops.mask_structure(mask, S)
    assert st == (1.0, 0.0, S - 1)
    da = (torch.randn(B, S, H, D, device=dev) * 0.02).to(torch.bfloat16)
    if head_scaled:      # query head j of a group weighs 2^(-10 j): the order of the group's sum shows in the bits
        w = torch.tensor([2.0 ** (-10 * (j % rep)) for j in range(H)], device=dev, dtype=torch.bfloat16)
        da = da * w[None, None, :, None]
    if cancel:           # ... and receives the negated gradient: a_j + a_(j+4) == 0 exactly, while an ascending sum leaves rounding residue
        dg = da.view(B, S, hk, rep, D)
        dg[:, :, :, 4:] = -dg[:, :, :, :4]
    ql, kl, vl = (t.detach().requires_grad_(True) for t in (q, k, v))
    ke = kl[:, :, None].expand(B, hk, rep, S, D).reshape(B, H, S, D) if rep > 1 else kl        # transformers' repeat_kv
    ve = vl[:, :, None].expand(B, hk, rep, S, D).reshape(B, H, S, D) if rep > 1 else vl
    o = F.scaled_dot_product_attention(ql, ke, ve, attn_mask=mask, dropout_p=0.0, is_causal=False, scale=scale)
    ao = o.transpose(1, 2).contiguous()
    grads = tuple(g.detach() for g in torch.autograd.grad(ao, (ql, kl, vl), da))
    with torch.no_grad():
        mo, mlse = ops.attn_fwd_exact(q, k, v, st, scale, key_block=ops.attn_key_block_guess(D, S))
    assert _ndiff(mo, ao.detach()) == 0
    return (q, k, v, mo, mlse, st), da, scale, grads


def _check(got, grads):
    for name, mine, ref in zip(("dq", "dk", "dv"), got, grads):
        assert tuple(mine.shape) == tuple(ref.shape), name
        assert _ndiff(mine, ref) == 0, name


@pytest.mark.parametrize("shape", [REP4, REP8, REP2], ids=["rep4-8-items", "rep8-seq384", "rep2-324-items"])
def test_grouped_kernel_has_autograds_bits(shape):
    from auto_round_amd import ops
    from auto_round_amd.exact_block import exact_attention_backward

    xa, da, scale, grads = _case(shape)
    with torch.no_grad():
        got = ops.attn_bwd_exact(*xa[:5], da, xa[5], scale, grouped=True)
        assert got is not None                                            # the persistent kernel took the call
        B, H, hk, S, D = shape
        assert tuple(got[1].shape) == (B, S, hk, D)
        _check(tuple(t.transpose(1, 2) for t in got), grads)
        _check(exact_attention_backward(xa, da, scale), grads)            # and the callers' function, which uses it


def test_ungrouped_heads_into_column_slices_of_a_wider_buffer():
    """kv_rep == 1 through the persistent kernel: results written directly, into column slices; what lies outside the slices stays"""
    from auto_round_amd import ops

    B, H, hk, S, D = REP1
    xa, da, scale, grads = _case(REP1)
    n = H * D
    wide = torch.full((B * S, 3 * n + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    outs = (wide[:, 8:8 + n], wide[:, 16 + n:16 + 2 * n], wide[:, 24 + 2 * n:24 + 3 * n])
    with torch.no_grad():
        got = ops.attn_bwd_exact(*xa[:5], da, xa[5], scale, dq=outs[0], dk=outs[1], dv=outs[2], grouped=True)
    assert got is not None
    for t, o in zip(got, outs):
        assert t.data_ptr() == o.data_ptr()
    _check(tuple(t.transpose(1, 2) for t in got), grads)
    for lo, hi in ((0, 8), (8 + n, 16 + n), (16 + 2 * n, 24 + 2 * n)):
        assert bool((wide[:, lo:hi] == 7.0).all())


@pytest.mark.parametrize("shape", [REP4, REP8], ids=["rep4", "rep8"])
def test_group_sum_order_is_torchs(shape):
    """dout of query head j scaled by 2^(-10 (j mod rep)): the addends of a group span 2^30 (rep 4) and more"""
    from auto_round_amd import ops

    xa, da, scale, grads = _case(shape, head_scaled=True)
    with torch.no_grad():
        got = ops.attn_bwd_exact(*xa[:5], da, xa[5], scale, grouped=True)
    assert got is not None
    _check(tuple(t.transpose(1, 2) for t in got), grads)


def test_pairs_of_a_group_of_eight_cancel_as_in_torch():
    """heads j and j + 4 of every group with equal queries and negated output gradients: their dk / dv contributions are exact
    negatives.  Summed as pairs first (torch's four accumulators) the group's gradient is exactly zero; summed in ascending order it is
    the rounding residue of heads whose sizes differ by 2^10 each.  Whatever torch returns, the kernel must return."""
    from auto_round_amd import ops

    xa, da, scale, grads = _case(REP8, head_scaled=True, cancel=True)
    with torch.no_grad():
        got = ops.attn_bwd_exact(*xa[:5], da, xa[5], scale, grouped=True)
    assert got is not None
    print("nonzero dk / dv values in torch's result:", int((grads[1] != 0).sum()), int((grads[2] != 0).sum()))
    _check(tuple(t.transpose(1, 2) for t in got), grads)


def test_head_size_64_with_grouping_takes_the_per_head_path():
    from auto_round_amd import ops
    from auto_round_amd.exact_block import exact_attention_backward

    shape = (2, 8, 2, 512, 64)
    xa, da, scale, grads = _case(shape, std=0.35)
    with torch.no_grad():
        assert ops.attn_bwd_exact(*xa[:5], da, xa[5], scale, grouped=True) is None
        _check(exact_attention_backward(xa, da, scale), grads)


def test_repeated_calls_alternating_shapes_are_identical():
    """ten calls at one shape, alternating with calls at another in the same process: stale LDS or workspace contents across units
    and calls would show"""
    from auto_round_amd.exact_block import exact_attention_backward

    cases = [_case(REP4), _case(REP8), _case(REP2)]            # ten calls at the first, alternating with the second (and the fourth shape)
    with torch.no_grad():
        first = [[t.clone() for t in exact_attention_backward(xa, da, scale)] for xa, da, scale, _ in cases]
        for i in range(10):
            for n in (0, 1 + i % 2):
                xa, da, scale, _ = cases[n]
                assert all(torch.equal(g, f) for g, f in zip(exact_attention_backward(xa, da, scale), first[n]))
