"""ar_attn_fwd_exact / ar_attn_bwd_exact / ar_attn_bwd_exact_grouped (csrc/ar_attn_exact.hip) at the edges of what their launchers
accept, against torch's own attention on the GPU (`F.scaled_dot_product_attention(q, repeat_kv(k), repeat_kv(v), attn_mask=<the dense
mask>)` under autograd -- the call transformers' `sdpa_attention_forward` makes under the reference's `block_forward`:
auto_round/compressors/utils.py:109-172), value for value: valid lengths on and around every 32- / 64-row boundary the kernels
classify tiles by, bias pairs other than (1, 0), the operand layouts the callers pass, group sizes 3, 6 and 1, and operand values in
the tails.  The cases come from tests/attn_exact_cases.py (tests/test_attn_exact_cases_host.py checks them on the host).

A case passes when O, LSE, dQ, dK and dV are torch's bit for bit.  On a difference every differing case is reported (never only the
first): per tensor the number of differing values, the (batch, head, row) of the first and the kernels' classes of the tiles along
that row, and both sides' largest error against a plain fp64 attention.  Torch's attention with an additive mask is itself not
perfectly reproducible (README), so a differing case computes torch's result a second time: two different results
of which the kernel equals one count as a library flake (printed; at most one per test function), anything else fails."""
import glob
import json
import os

import pytest
import torch
import torch.nn.functional as F

import attn_exact_cases as xc

pytestmark = pytest.mark.gpu

NAMES = ("o", "lse", "dq", "dk", "dv")
_operand_cache: dict = {}


def _operands(c):
    key = (c.shape, c.layout, c.family, c.head_scaled)
    if key not in _operand_cache:
        if len(_operand_cache) > 2:
            _operand_cache.clear()
        _operand_cache[key] = xc.operands(c, device="cuda")
    return _operand_cache[key]


def _repeat_kv(t, rep):
    B, hk, S, D = t.shape
    return t[:, :, None].expand(B, hk, rep, S, D).reshape(B, hk * rep, S, D) if rep > 1 else t        # transformers' repeat_kv


def _torch_reference(x, mask, scale):
    """torch's result for the call, on the same views: (o [B, H, S, D], lse [B, H, S], dq [B, H, S, D], dk, dv [B, hk, S, D])"""
    q, k, v = x["q"], x["k"], x["v"]
    B, H, S, D = q.shape
    rep = H // k.shape[1]
    ql, kl, vl = (t.detach().requires_grad_(True) for t in (q, k, v))
    ke, ve = _repeat_kv(kl, rep), _repeat_kv(vl, rep)
    o = F.scaled_dot_product_attention(ql, ke, ve, attn_mask=mask, dropout_p=0.0, is_causal=False, scale=scale)
    ao = o.transpose(1, 2).contiguous()
    gq, gk, gv = torch.autograd.grad(ao, (ql, kl, vl), x["dout"])
    with torch.no_grad():
        lse = torch.ops.aten._scaled_dot_product_efficient_attention(q, ke.detach(), ve.detach(), mask.expand(B, H, S, S), True, 0.0, False,
                                                                     scale=scale)[1][..., :S]
    return o.detach(), lse, gq, gk, gv


def _callers_backward(x):
    from auto_round_amd.exact_block import exact_attention_backward

    return lambda xa, da, scale: exact_attention_backward(xa, da, scale, outs=x["outs"])


def _kernels(x, st, scale, backward):
    from auto_round_amd import ops

    q, k, v = x["q"], x["k"], x["v"]
    S, D = int(q.shape[2]), int(q.shape[3])
    with torch.no_grad():
        got = ops.attn_fwd_exact(q, k, v, st, scale, key_block=ops.attn_key_block_guess(D, S))
        assert got is not None, "the forward refused a case of the tables"
        mo, mlse = got
        grads = backward((q, k, v, mo, mlse, st), x["dout"], scale)
        assert grads is not None, "the backward refused a case of the tables"
    return (mo.transpose(1, 2), mlse) + tuple(grads)


def _diff(a, b):
    """(number of values whose bits differ, index of the first) of two tensors of one shape"""
    assert tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    a, b = a.contiguous(), b.contiguous()
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    ne = (a.view(it) != b.view(it)).flatten()
    n = int(ne.sum())
    return n, (tuple(int(i) for i in torch.unravel_index(ne.int().argmax(), a.shape)) if n else None)


def _same(xs, ys):
    return all(_diff(a, b)[0] == 0 for a, b in zip(xs, ys))


def _report(c, x, mask, scale, got, ref, diffs):
    S = c.shape[3]
    f64 = dict(zip(NAMES, xc.fp64_attention(x["q"], x["k"], x["v"], mask, scale, x["dout"])))
    f64["o"] = f64["o"].transpose(1, 2)
    lines = [f"shape {c.shape} valid {c.valid} bias {c.bias} layout {c.layout} values {c.family}{' head-scaled dout' if c.head_scaled else ''}:"]
    for name, g, r, (n, first) in zip(NAMES, got, ref, diffs):
        if not n:
            continue
        b, h, row = first[:3]
        key_side = name in ("dk", "dv")
        qs, ks = xc.tile_class(row, row, c.valid)
        lines.append(f"  {name}: {n} of {g.numel()} values differ; first at (batch {b}, head {h}, row {row}); tiles along that "
                     f"{'key row (MODE 1)' if key_side else 'query row (forward / MODE 0)'}: {xc.row_classes(row, S, c.valid, key_side)}, the diagonal's: "
                     f"{ks if key_side else qs}; largest error against fp64: kernel {float((g.double() - f64[name]).abs().max()):.3e}, "
                     f"torch {float((r.double() - f64[name]).abs().max()):.3e}")
    return "\n".join(lines)


def _versions():
    lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    aot = sorted(os.path.basename(p).split(".so.")[-1] for p in glob.glob(os.path.join(lib, "libaotriton*.so.*")))
    return {"torch": torch.__version__, "aotriton": aot[-1] if aot else None}


def _run(test_id, backward=None, after=None):
    """every case of a table through the kernels and through torch; the record of the run is printed as one `EDGE_RECORD` line"""
    from auto_round_amd import ops

    cases = xc.all_tables()[test_id]
    failures, flakes, differing, max_scores = [], [], dict.fromkeys(NAMES, 0), {}
    for c in cases:
        B, H, hk, S, D = c.shape
        scale = xc.SETTINGS[D][0]
        x = _operands(c)
        mask = xc.dense_mask(B, S, c.valid, *c.bias, device="cuda")
        st = ops.mask_structure(mask, S)
        assert st == (c.bias[0], c.bias[1], c.valid), c
        if x["wide"] is not None:
            x["wide"].fill_(7.0)
        got = _kernels(x, st, scale, backward(x) if backward else _callers_backward(x))
        if after:
            after(c, x, got)
        ref = _torch_reference(x, mask, scale)
        diffs = [_diff(g, r) for g, r in zip(got, ref)]
        max_scores[f"{c.shape}"] = round(x["max_score"], 3)
        if any(n for n, _ in diffs):
            again = _torch_reference(x, mask, scale)
            if not _same(ref, again) and _same(got, again):
                flakes.append(f"library flake: shape {c.shape} valid {c.valid} bias {c.bias} layout {c.layout} values {c.family}: torch's two "
                              f"results differ from each other ({[_diff(a, b)[0] for a, b in zip(ref, again)]} values) and the kernels equal the second")
                continue
            for name, (n, _) in zip(NAMES, diffs):
                differing[name] += n
            failures.append(_report(c, x, mask, scale, got, ref, diffs))
    for line in flakes:
        print(line)
    print("EDGE_RECORD " + json.dumps({"test": test_id, "cases": len(cases), "differing_values": differing, "failed_cases": len(failures),
                                       "library_flakes": len(flakes), "largest_score": max_scores, **_versions()}))
    assert not failures, f"{len(failures)} of {len(cases)} cases differ from torch:\n" + "\n".join(failures)
    assert len(flakes) <= 1, "more than one library flake in one test:\n" + "\n".join(flakes)


# a. valid lengths on, one under and one over every 32- / 64-row boundary, bias (1, 0), at the smallest shape that selects each kernel form
@pytest.mark.parametrize("name", list(xc.GRID_SHAPES))
def test_valid_length_grid(name):
    _run("grid/" + name)


@pytest.mark.parametrize("name", list(xc.REFUSED_SHAPES))
def test_head_size_64_at_128_tokens_is_refused(name):
    """the row of the valid-length grid at which the backward was found NOT to have torch's bits (1 to 9 of 32768 dq / dk / dv values at
    every valid length; the forward did): both launchers refuse the shape, at every valid length, and the caller keeps torch's SDPA"""
    from auto_round_amd import ops
    from auto_round_amd.exact_block import exact_attention_forward

    cases = xc.all_tables()["refused/" + name]
    for c in cases:
        B, H, hk, S, D = c.shape
        scale = xc.SETTINGS[D][0]
        x = _operands(c)
        mask = xc.dense_mask(B, S, c.valid, *c.bias, device="cuda")
        st = ops.mask_structure(mask, S)
        assert st == (c.bias[0], c.bias[1], c.valid), c
        o, lse = _torch_reference(x, mask, scale)[:2]
        with torch.no_grad():
            for kb in (0, 16, 32, 64):
                assert ops.attn_fwd_exact(x["q"], x["k"], x["v"], st, scale, key_block=kb) is None, c
            assert exact_attention_forward(x["q"], x["k"], x["v"], mask, scale, S) is None, c
            for grouped in (False, True):
                assert ops.attn_bwd_exact(x["q"], x["k"], x["v"], o.transpose(1, 2).contiguous(), lse.contiguous(), x["dout"], st, scale,
                                          grouped=grouped) is None, c
    print("EDGE_RECORD " + json.dumps({"test": "refused/" + name, "cases": len(cases), "refused": len(cases), **_versions()}))


# b. every bias pair at valid 1, S / 2 + 1 and S: (3, -2.5) and (0.8125, -0.0078125) tell `bias * (1 / sm_scale)` from `bias / sm_scale`
# in the backward and exercise the forward's bf16 rounding of `bias * log2 e`
@pytest.mark.parametrize("name", list(xc.BIAS_SHAPES))
def test_bias_pairs(name):
    _run("bias/" + name)


# c. the layouts the callers pass (the reference call gets the same views)
@pytest.mark.parametrize("layout", ["head_major", "qkv_slices", "dout_slice"])
def test_operand_layouts(layout):
    _run("layout/" + layout)


def test_gradients_into_column_slices_of_a_wider_buffer():
    """dq / dk / dv through `outs=` into column slices of one gradient buffer filled with 7.0, at groups of 4, 8 and 1: the results are
    written there, and what lies outside the slices stays"""

    def after(c, x, got):
        for g, o in zip(got[2:], x["outs"]):
            assert g.data_ptr() == o.data_ptr(), c
        for lo, hi in x["gaps"]:
            assert bool((x["wide"][:, lo:hi] == 7.0).all()), (c, lo, hi)

    _run("layout/outs_slices", after=after)


# d. group sizes
def _grouped_call(expect_taken):
    def backward(x):
        from auto_round_amd import ops

        def run(xa, da, scale):
            got = ops.attn_bwd_exact(*xa[:5], da, xa[5], scale, grouped=True)
            if not expect_taken:
                assert got is None, "the grouped kernel took a group size it does not restate"
                return _callers_backward(x)(xa, da, scale)          # the per-head kernel and torch's sum over the group
            assert got is not None, "the grouped kernel refused the call"
            H, hk = xa[0].shape[1], xa[1].shape[1]
            assert got[1].shape[2] == hk and got[2].shape[2] == hk and got[0].shape[2] == H
            res = tuple(t.transpose(1, 2) for t in got)
            assert _same(res, _callers_backward(x)(xa, da, scale))  # and the callers' function returns the same
            return res

        return run

    return backward


@pytest.mark.parametrize("name", ["rep3", "rep1-grouped", "rep3-head-scaled"])
def test_group_sizes_the_grouped_kernel_takes(name):
    _run("group/" + name, backward=_grouped_call(True))


def test_group_of_six_is_refused_and_summed_by_torch():
    _run("group/rep6", backward=_grouped_call(False))


# e. operand values in the tails: an attention sink, saturated scores, rows of zeros
@pytest.mark.parametrize("family", list(xc.VALUE_FAMILIES))
def test_operand_value_families(family):
    _run("values/" + family)
    for shape in xc.VALUE_SHAPES:
        print(f"{family} {shape}: largest score {_operands(xc._case(shape, shape[3] - 1, family=family))['max_score']:.3f}")

