"""The case tables of tests/attn_exact_cases.py, checked on the host: every case the GPU edge tests (tests/test_gpu_attn_exact_edges.py)
run is one `ops.mask_structure` recognises, with bias values that are bf16 numbers and operand layouts the launchers' ABI takes -- so
no GPU case can be refused (and silently test nothing) for a reason that lies in the tables."""
import pytest
import torch

import attn_exact_cases as xc
from auto_round_amd import ops

TABLES = xc.all_tables()


def test_the_tables_hold_the_planned_cases():
    assert xc.valid_grid(384) == [1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, 319, 320, 321, 351, 352, 383, 384]
    assert xc.valid_grid(128) == [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128]
    assert len(xc.BIAS_PAIRS) == 7 and len(set(xc.BIAS_PAIRS)) == 7
    assert sorted(TABLES) == sorted(["grid/" + n for n in xc.GRID_SHAPES] + ["refused/" + n for n in xc.REFUSED_SHAPES] + ["bias/" + n for n in xc.BIAS_SHAPES]
                                    + ["layout/" + n for n in xc.LAYOUTS] + ["group/" + n for n in xc.GROUP_CASES]
                                    + ["values/" + n for n in xc.VALUE_FAMILIES])
    for name, cases in TABLES.items():
        assert cases and len(set(cases)) == len(cases), name
        if name.startswith(("grid/", "refused/")):
            assert len(cases) == len(xc.valid_grid(cases[0].shape[3]))
        if name.startswith("bias/"):
            assert len(cases) == 21
    for shape in {c.shape for cases in TABLES.values() for c in cases}:
        B, H, hk, S, D = shape
        assert D in xc.SETTINGS and S % 128 == 0 and H % hk == 0
        assert D == 64 or S > 256                        # head size 128 at S <= 256 is not claimed
        assert (D == 64 and S < 256) == (shape in xc.REFUSED_SHAPES.values())          # head size 64 at S = 128 is refused


@pytest.mark.parametrize("name", sorted(TABLES))
def test_every_case_is_one_mask_structure_recognises(name):
    for c in TABLES[name]:
        B, H, hk, S, D = c.shape
        for b in c.bias:
            assert float(torch.tensor(b, dtype=torch.float32).to(torch.bfloat16)) == b, c        # a bf16 number
            assert abs(b) <= 1e4
        assert 1 <= c.valid <= S
        st = ops.mask_structure(xc.dense_mask(B, S, c.valid, *c.bias), S)
        assert st == (c.bias[0], c.bias[1], c.valid), c


@pytest.mark.parametrize("name", sorted(TABLES))
def test_every_layout_is_one_the_abi_takes(name):
    seen = set()
    for c in TABLES[name]:
        if (c.shape, c.layout) in seen:                   # (the layout depends on neither the mask nor the values)
            continue
        seen.add((c.shape, c.layout))
        B, H, hk, S, D = c.shape
        x = xc.operands(c)
        assert tuple(x["q"].shape) == (B, H, S, D) and tuple(x["k"].shape) == (B, hk, S, D) and tuple(x["v"].shape) == (B, hk, S, D)
        assert tuple(x["dout"].shape) == (B, S, H, D)
        for key in ("q", "k", "v", "dout"):
            t = x[key]
            assert t.dtype == torch.bfloat16 and t.stride(3) == 1 and all(s % 8 == 0 for s in t.stride()[:3]), (c, key, t.stride())
            base = t.data_ptr() - t.storage_offset() * t.element_size()
            assert base % 16 == 0 and (t.storage_offset() * t.element_size()) % 16 == 0, (c, key)
        if c.layout == "head_major":
            assert all(x[key].is_contiguous() for key in ("q", "k", "v"))
        if c.layout == "qkv_slices":
            assert len({x[key].untyped_storage().data_ptr() for key in ("q", "k", "v")}) == 1
            assert x["q"].storage_offset() == 8 and x["q"].stride(2) == (H + 2 * hk) * D + 16
        if c.layout == "dout_slice":
            assert x["dout"].storage_offset() == 8 and x["dout"].stride(1) == H * D + 16 and not x["dout"].is_contiguous()
        if c.layout == "outs_slices":
            wide = x["wide"]
            covered = torch.zeros(wide.shape[1], dtype=torch.int32)
            for t, nh in zip(x["outs"], (H, hk, hk)):
                assert tuple(t.shape) == (B * S, nh * D) and t.stride(1) == 1 and t.stride(0) % 8 == 0
                assert (t.storage_offset() * t.element_size()) % 16 == 0
                covered[t.storage_offset():t.storage_offset() + nh * D] += 1
            for lo, hi in x["gaps"]:
                covered[lo:hi] += 1
            assert bool((covered == 1).all())             # slices and gaps tile the buffer's columns
            assert bool((wide == 7.0).all())
        else:
            assert x["outs"] is None


def test_operand_values_do_not_depend_on_the_layout():
    base = xc.operands(xc._case(xc.LAYOUT_SHAPES[2], 100))
    for layout in xc.LAYOUTS:
        x = xc.operands(xc._case(xc.LAYOUT_SHAPES[2], 100, layout=layout))
        assert all(torch.equal(x[key], base[key]) for key in ("q", "k", "v", "dout")), layout


def test_value_families_reach_what_they_are_for():
    for shape in xc.VALUE_SHAPES:
        B, H, hk, S, D = shape
        plain = xc.operands(xc._case(shape, S - 1))["max_score"]
        sink = xc.operands(xc._case(shape, S - 1, family="sink"))
        assert sink["max_score"] > 30.0 and sink["max_score"] > 4 * plain
        assert 20.0 < xc.operands(xc._case(shape, S - 1, family="sink_mild"))["max_score"] < 100.0          # several tens
        assert xc.operands(xc._case(shape, S - 1, family="saturation"))["max_score"] > 8 * plain
        deg = xc.operands(xc._case(shape, S - 1, family="degenerate"))
        q = deg["q"].float()
        assert bool((q[:, :, 80:144] == 0).all()) and not bool(torch.signbit(q[:, :, 80:112]).any()) and bool(torch.signbit(q[:, :, 112:144]).all())
        assert bool((deg["dout"][:, :, H - 1] == 0).all()) and bool((deg["dout"][:, :, 0] != 0).any())


@pytest.mark.parametrize("S", sorted({c.shape[3] for cases in TABLES.values() for c in cases}))
def test_tile_class_agrees_with_the_dense_mask(S):
    """`plain` exactly where every pair of the tile is kept, `all_out` exactly where none is -- for both tilings, at every valid length used"""
    valids = sorted({c.valid for cases in TABLES.values() for c in cases if c.shape[3] == S})
    idx = torch.arange(S)
    for valid in valids:
        keep = (idx[None, :] <= idx[:, None]) & (idx[None, :] < valid)                       # [query, key]
        for side, (qb, kb) in enumerate(((32, 64), (64, 32))):                              # forward / MODE 0, MODE 1
            n = keep.view(S // qb, qb, S // kb, kb).sum((1, 3))
            for i in range(S // qb):
                for j in range(S // kb):
                    want = "plain" if n[i, j] == qb * kb else "all_out" if n[i, j] == 0 else "mixed"
                    assert xc.tile_class(i * qb, j * kb, valid)[side] == want, (S, valid, side, i, j)
                    assert xc.tile_class(i * qb + qb - 1, j * kb + kb - 1, valid)[side] == want


def test_fp64_attention_is_plain_attention():
    c = xc._case((1, 4, 2, 128, 64), 100, bias=(0.5, -2.0))
    x = xc.operands(c)
    mask = xc.dense_mask(1, 128, c.valid, *c.bias)
    o, lse, dq, dk, dv = xc.fp64_attention(x["q"], x["k"], x["v"], mask, 1.0, x["dout"])
    assert o.dtype == torch.float64 and tuple(o.shape) == (1, 128, 4, 64) and tuple(lse.shape) == (1, 4, 128)
    assert tuple(dq.shape) == (1, 4, 128, 64) and tuple(dk.shape) == (1, 2, 128, 64) and tuple(dv.shape) == (1, 2, 128, 64)
    # one row by hand: query 5 of head 3 (key head 1)
    q, k, v = x["q"].double()[0, 3, 5], x["k"].double()[0, 1], x["v"].double()[0, 1]
    s = k @ q + mask.double()[0, 0, 5]
    p = torch.exp(s - s.max())
    assert torch.allclose(o[0, 5, 3], (p / p.sum()) @ v, rtol=1e-12, atol=1e-14)
    assert torch.allclose(lse[0, 3, 5], s.max() + torch.log(p.sum()), rtol=1e-12, atol=0)
