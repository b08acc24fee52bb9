"""`exact_rounding` for OPT-style decoder blocks (round 6; BASELINE configs[0] / the north-star's own model, OPT-125M): the block the
reference tunes through transformers' EAGER module code (auto_round/compressors/utils.py:109-172 `block_forward` around
transformers/models/opt/modeling_opt.py `OPTDecoderLayer` / `OPTAttention`) run as ONE autograd node with the module path's bits.

What the module path computes, op by op (eval mode: the dropouts are identities), and what runs here:

  self_attn_layer_norm / final_layer_norm   under autocast `layer_norm` is on torch's fp32 list: x.float() -> native_layer_norm in fp32
                                            -> the consuming linear casts to bf16.  Here: csrc/ar_exact_ln.hip, ATen's vectorised
                                            kernel restated (per-thread Welford over float4 vectors, shuffle-down combine over the
                                            64-lane wavefront, shared-memory combine over the 4 wavefronts; backward: two block
                                            sums in ATen's association) with the two casts folded in -- or, where that kernel does
                                            not prove bit-equal, torch's own ops in a local autograd graph.
  q_proj / k_proj / v_proj, out_proj,       `F.linear(x, Wq, bias)` exactly as `wrapper._QLinearFn` issues it, one call per layer (the
  fc1, fc2                                  library's bias epilogue included); weight gradients `torch.mm(dY^T, X)` into the arena,
                                            input gradients `torch.mm(dY, Wq)` -- the module path's own calls.
  q_proj(x) * scaling                       torch's multiply by a python scalar (its own rounding), backward the same.
  attention                                 transformers' `sdpa_attention_forward` on the layouts `OPTAttention` hands over
                                            (scaling = 1.0), in a local autograd graph: the library kernels the module path calls --
                                            or (round 6, option `attn`) csrc/ar_attn_exact.hip, the library attention's arithmetic
                                            restated from torch's gfx950 code objects: the same bits at 0.59 instead of 1.46 ms,
                                            and without the library forward's run-to-run slips at head size 64.
  residual adds, ReLU                       torch's add / relu / threshold_backward: one rounding each, as eager.

Nothing is assumed: `plan_against_module` runs real minibatches forward + backward through the module code and through this class on
the same frozen state and compares the block output and every weight gradient bit for bit -- first with every segment on torch's own
ops, then with each LayerNorm kernel switched on, kept only after two consecutive runs without a differing value.  What is gained over
the module path is launches and host work, not arithmetic: one autograd node instead of ~25, no module dispatch, no dtype-conversion
kernels around the norms (measured at OPT-125M, full recipe: 3.27 ms per iteration against the module path's 3.48; the loop is then
GPU-bound, 88 % of it the library attention and GEMMs whose bits are the reference's -- profiles/r06_opt125m_exact_kernel_stats.csv)."""
from __future__ import annotations

import contextlib
import warnings
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from . import ops
from .exact_proof import ExactBlockMixin, Proof, attention_forward_same, bits_equal, key_block_candidates
from .fused_block import OPT_FAMILY, FusedOPTBlock, _class_in

GEMM_OPTS = ("merged_qkv", "dw_qkv")      # q / k / v as ONE library GEMM forward (N = 3 H) and ONE weight-gradient GEMM -- kept when bit-equal
KERNEL_OPTS = ("ln1", "ln2", "attn")     # "attn": csrc/ar_attn_exact.hip instead of torch's SDPA (exact_proof.py)
# flag bits of the LayerNorm kernels that an installed torch build may resolve either way (csrc/ar_exact_ln.hip): tried in this order
LN_VARIANTS = (0, 1, 2, 3)


class ExactOPTBlock(ExactBlockMixin, FusedOPTBlock):
    # -- construction -------------------------------------------------------------------------------------------------------
    @classmethod
    def try_build(cls, block, arenas, input_others, amp_dtype=torch.bfloat16, sdpa_ctx=None, amp=True, **_) -> Optional["ExactOPTBlock"]:
        if not _class_in(block, OPT_FAMILY):
            return None
        self = super().try_build(block, arenas, input_others, amp_dtype, sdpa_ctx=sdpa_ctx, use_mfma_dw=False, tn_dx_gemm=False)
        if self is None or not self._usable():
            return None
        self._init_exact_state(amp)
        return self

    @classmethod
    def try_build_plain(cls, block, input_others, amp_dtype=torch.bfloat16, sdpa_ctx=None, amp=True) -> Optional["ExactOPTBlock"]:
        """The no-grad form for an UNWRAPPED block (targets, quantised-output forward): same kernels, forward-only proof."""
        if not _class_in(block, OPT_FAMILY):
            return None
        self = super().try_build_plain(block, input_others, amp_dtype, sdpa_ctx=sdpa_ctx)
        if self is None or not self._usable():
            return None
        attn = self.attn
        self._init_exact_state(amp, plain=dict(q=attn.q_proj, k=attn.k_proj, v=attn.v_proj, o=attn.out_proj, f1=block.fc1, f2=block.fc2))
        return self

    def _usable(self) -> bool:
        if getattr(getattr(self.attn, "config", None), "_attn_implementation", None) != "sdpa":
            return False
        n1, n2 = self.n1, self.n2
        if any(n.bias is None or n.weight.dtype != self.dtype or n.bias.dtype != self.dtype or tuple(n.normalized_shape) != (self.H,)
               for n in (n1, n2)):
            return False
        # activation-quantised schemes: under autocast the module path fake-quantises the LayerNorm's FP32 output (each WrapperLinear
        # quantises the tensor it is handed, and the cast to the activation dtype happens inside its linear); this class hands the
        # norm's output over in the activation dtype -- other quantisation inputs, so those blocks keep the module path
        if self.aq.get("qkv") is not None or self.aq.get("f1") is not None:
            return False
        return not self.block.training

    @staticmethod
    def base_plan() -> Dict[str, object]:
        """every segment on torch's own ops (exact by construction)"""
        return dict(ln1=False, ln2=False, ln_flags=0, attn=False, attn_kb=0, merged_qkv=False, dw_qkv=False)

    def set_plan(self, plan):
        self.plan = {**self.base_plan(), **plan}

    def _refresh_tn(self):      # (the fused class's transposed dX weights are not used here)
        pass

    def _dw_x(self, key, dY2d, X2d):
        """dW of layer `key` into the arena exactly as `_QLinearFn.backward` issues it (the library GEMM; `addmm_` when micro-batches
        accumulate)"""
        lyr = self.layers[key]
        if lyr._dw_accum[0]:
            lyr.weight_grad.addmm_(dY2d.t(), X2d)
        else:
            torch.mm(dY2d.t(), X2d, out=lyr.weight_grad)
        self._dw_written((lyr,))

    def _ln_module(self, norm, x2d, B, S, grad):
        """the module code's LayerNorm on torch's ops: under autocast an fp32 `layer_norm` whose result the consuming linear casts to
        the activation dtype -> (h [T, H] in the activation dtype, (leaf, graph output) for the backward or None)"""
        with torch.enable_grad() if grad else contextlib.nullcontext():
            xl = x2d.detach().requires_grad_(grad)
            with self._ctx(S):
                hg = norm(xl.view(B, S, self.H))
            hg = hg.reshape(B * S, self.H)
            if hg.dtype != self.dtype:
                hg = hg.to(self.dtype)
        return hg.detach(), ((xl, hg) if grad else None)

    # -- forward -------------------------------------------------------------------------------------------------------------
    def _forward_impl(self, x, others, ctx):
        from .wrapper import act_quant_fwd_raw

        P, L, aq = self.plan, self.layers, self.aq
        grad = ctx is not None
        B, S, H = x.shape
        T = B * S
        hq, hd = self.hq, self.hd
        x2d = x.reshape(T, H)
        if x2d.dtype != self.dtype:
            x2d = x2d.to(self.dtype)
        x2d = x2d.contiguous()

        def fq(t, plan):
            return t if plan is None else act_quant_fwd_raw(t, plan)

        # self_attn_layer_norm (the block input needs no gradient)
        res = ops.layernorm_fwd_exact(x2d, self.n1.weight, self.n1.bias, float(self.n1.eps), flags=int(P["ln_flags"]), want_stats=False) if P["ln1"] else None
        h1 = res[0] if res is not None else self._ln_module(self.n1, x2d, B, S, False)[0]
        h1_in = fq(h1, aq["qkv"])
        if P.get("merged_qkv"):      # one GEMM over the three projections' rows (adjacent in the arena): column slices go on
            qkv = F.linear(h1_in, self.Wqkv, self.b_qkv)
            at = {n: i * H for i, n in enumerate(self.order)}
            q2d = qkv[:, at["q"]:at["q"] + H] * self.qscale
            k2d, v2d = qkv[:, at["k"]:at["k"] + H], qkv[:, at["v"]:at["v"] + H]
            del qkv
        else:
            q2d = F.linear(h1_in, L["q"].weight_q, self._bias("q")) * self.qscale         # OPTAttention: q_proj(x) * scaling
            k2d = F.linear(h1_in, L["k"].weight_q, self._bias("k"))
            v2d = F.linear(h1_in, L["v"].weight_q, self._bias("v"))
        q4, k4, v4 = (t.view(B, S, hq, hd).transpose(1, 2) for t in (q2d, k2d, v2d))
        a2d, attn_saved = self._attention_forward(q4, k4, v4, others.get("attention_mask"), 1.0, grad)      # (q is scaled already)
        del q2d, k2d, v2d
        a_in = fq(a2d, aq["o"])
        x2 = x2d + F.linear(a_in, L["o"].weight_q, self._bias("o"))                   # residual + out_proj(attn)
        # final_layer_norm
        norm_graph, mean2, rstd2 = None, None, None
        res = ops.layernorm_fwd_exact(x2, self.n2.weight, self.n2.bias, float(self.n2.eps), flags=int(P["ln_flags"]), want_stats=grad) if P["ln2"] else None
        if res is not None:
            h2, mean2, rstd2 = res
        else:
            h2, norm_graph = self._ln_module(self.n2, x2, B, S, grad)
        h2_in = fq(h2, aq["f1"])
        a = torch.relu_(F.linear(h2_in, L["f1"].weight_q, self._bias("f1")))         # nn.ReLU()(fc1(.)): same values, in place
        f_in = fq(a, aq["f2"])
        y = x2 + F.linear(f_in, L["f2"].weight_q, self._bias("f2"))
        if grad:
            ctx.saved = dict(B=B, S=S, h1_in=h1_in, h1=h1, attn=attn_saved, a2d=a2d, a_in=a_in, x2=x2, mean2=mean2, rstd2=rstd2,
                             norm_graph=norm_graph, h2=h2, h2_in=h2_in, a=a, f_in=f_in)
        return y.view(B, S, H)

    # -- backward ------------------------------------------------------------------------------------------------------------
    def _backward_impl(self, ctx, dy):
        from .wrapper import act_quant_bwd_raw

        s = ctx.saved
        ctx.saved = None
        P, L, aq = self.plan, self.layers, self.aq
        B, S = s["B"], s["S"]
        T, H = B * S, self.H

        def bq(g, x, plan):
            return g if plan is None else act_quant_bwd_raw(g, x, plan)

        dy2d = dy.reshape(T, H)
        if dy2d.dtype != self.dtype:
            dy2d = dy2d.to(self.dtype)
        dy2d = dy2d.contiguous()
        # y = x2 + fc2(relu(fc1(ln2(x2))))
        self._dw_x("f2", dy2d, s.pop("f_in"))
        a = s.pop("a")
        da = bq(torch.mm(dy2d, L["f2"].weight_q), a, aq["f2"])
        df = torch.ops.aten.threshold_backward(da, a, 0)         # ReluBackward0
        del da, a
        self._dw_x("f1", df, s.pop("h2_in"))
        dh2 = bq(torch.mm(df, L["f1"].weight_q), s.pop("h2"), aq["f1"])
        del df
        norm_graph = s.pop("norm_graph")
        x2 = s.pop("x2")
        if norm_graph is None:
            dx2 = ops.layernorm_bwd_exact(dh2, x2, self.n2.weight, s.pop("mean2"), s.pop("rstd2"), dres=dy2d, flags=int(P["ln_flags"]), out=dh2)
        else:
            xl, hg = norm_graph
            (gx,) = torch.autograd.grad(hg, xl, dh2)
            dx2 = gx + dy2d            # the two uses of x2 (norm input, residual): autograd's accumulation, one rounding
        del dh2, norm_graph, x2
        # x2 = x + out_proj(attn)
        self._dw_x("o", dx2, s.pop("a_in"))
        dattn = bq(torch.mm(dx2, L["o"].weight_q), s.pop("a2d"), aq["o"])
        del dx2
        attn_saved = s.pop("attn")
        dqkv = torch.empty((T, 3 * H), dtype=self.dtype, device=dy2d.device) if P.get("dw_qkv") else None
        outs = None
        if dqkv is not None:
            at = {n: i * H for i, n in enumerate(self.order)}
            outs = tuple(dqkv[:, at[n]:at[n] + H] for n in "qkv")
        first_party = attn_saved[2] is not None
        gq4, gk4, gv4 = self._attention_backward(attn_saved, dattn, B, S, 1.0, outs=outs)
        del attn_saved, dattn
        h1_in = s.pop("h1_in")
        if dqkv is not None:          # the merged gradient buffer: one weight-gradient GEMM over the three projections' rows
            if not first_party:
                for n, g in zip("qkv", (gq4, gk4, gv4)):
                    outs["qkv".index(n)].view(B, S, self.hq, self.hd).copy_(g.transpose(1, 2))
            outs[0].mul_(self.qscale)                                  # MulBackward0 of q_proj(x) * scaling (its own rounding)
            acc = [l._dw_accum[0] for l in self.trio]
            if all(acc):
                self.dWqkv.addmm_(dqkv.t(), h1_in)
            elif not any(acc):
                torch.mm(dqkv.t(), h1_in, out=self.dWqkv)
            else:
                raise RuntimeError("q / k / v weight gradients in different accumulation states")
            self._dw_written(self.trio)
            return
        dq2d = gq4.transpose(1, 2).reshape(T, H) * self.qscale        # MulBackward0 of q_proj(x) * scaling
        dk2d = gk4.transpose(1, 2).reshape(T, H)
        dv2d = gv4.transpose(1, 2).reshape(T, H)
        self._dw_x("q", dq2d, h1_in)
        self._dw_x("k", dk2d, h1_in)
        self._dw_x("v", dv2d, h1_in)

    # -- the proof -------------------------------------------------------------------------------------------------------------
    def _ln_stats_match(self, x, flags) -> bool:
        """the LayerNorm kernel's fp32 row statistics and output against torch's own ops on the probe minibatch (a bf16 output
        alone could hide a last-bit difference in mean / rstd)"""
        x2d = x.reshape(-1, x.shape[-1]).to(self.dtype).contiguous()
        res = ops.layernorm_fwd_exact(x2d, self.n1.weight, self.n1.bias, float(self.n1.eps), flags=flags, want_stats=True)
        if res is None:
            return False
        xf = x2d.float()
        y, mean, rstd = torch.ops.aten.native_layer_norm(xf, [self.H], self.n1.weight.float(), self.n1.bias.float(), float(self.n1.eps))
        return bits_equal(res[1], mean.view(-1)) and bits_equal(res[2], rstd.view(-1)) and bits_equal(res[0], y.to(self.dtype))

    def plan_against_module(self, module_forward, x, others, ref, want=None, second=None) -> Optional[dict]:
        """Same contract as ExactLlamaBlock.plan_against_module, same rule (exact_proof.Proof): -> the proven plan (installed), or None
        when not even the all-torch form reproduces the module path (the caller keeps the module path).  An option joins the plan after TWO consecutive runs
        without a differing value (the second on `second`'s minibatch); one more pair is granted after a failed pair -- the library
        attention under the comparison slips about once in 4000 calls at this shape (profiles/r06_opt_loop_flake2.json)."""
        proof = Proof(self, module_forward, [(x, others, ref)] + ([second] if second is not None else []))
        report, proven = proof.report, proof.proven
        plan = self.base_plan()
        ok, n_bad = proven(plan)
        if not ok:          # once more: the comparison itself sits on a library that slips now and then
            ok, n_bad2 = proven(plan)
            if ok:
                report.setdefault("kept_on_second_try", []).append("base")
                warnings.warn(f"exact_rounding: {type(self.block).__name__}: the all-torch form differed from the module path in its first pair "
                              f"of runs ({n_bad} values) and matched in the second pair -- the library under the comparison is not perfectly repeatable")
        if not ok:
            return proof.refuse(n_bad)
        # the LayerNorm kernels: which of the build-dependent forms (fast reciprocal, contraction, rsqrt) reproduces torch's statistics
        flags = next((f for f in LN_VARIANTS if self._ln_stats_match(x, f)), None)
        for opt in [o for o in KERNEL_OPTS if want is None or o in want]:
            if opt == "attn" and others.get("attention_mask") is None:
                report["skipped"][opt] = "no additive attention mask: the call is not the one the kernel restates"
                continue
            report["tried"].append(opt)
            if flags is None and opt != "attn":
                report["errors"][opt] = "no form of the LayerNorm kernel reproduces torch's row statistics / output on this stack"
                report["dropped"][opt] = {"stats": "differ"}
                continue
            trials = [dict(plan, **{opt: True, "ln_flags": flags})]
            if opt == "attn":       # the library picks its forward configuration by shape: the measured guess first, then the other key blocks
                trials = [dict(plan, attn=True, attn_kb=kb) for kb in key_block_candidates(ops.attn_key_block_guess(self.hd, int(x.shape[1])))]
            worst = {}
            for attempt, trial in [(0, t) for t in trials] + [(1, trials[0])]:
                if opt in report["kept"]:
                    break
                ok, n_bad = proof.proven_attention(trial, attn_kb=trial["attn_kb"]) if opt == "attn" else proven(trial)
                if ok:
                    plan = trial
                    report["kept"].append(opt)
                    if attempt:
                        proof.kept_on_second_try(opt, worst)
                    break
                worst[f"{attempt}:{trial.get('attn_kb', 0)}" if opt == "attn" else str(attempt)] = n_bad
            if opt not in report["kept"]:
                report["dropped"][opt] = worst
        for opt in [o for o in GEMM_OPTS if want is None or o in want]:
            report["tried"].append(opt)
            trial = dict(plan, **{opt: True})
            worst = {}
            for attempt in (0, 1):
                ok, n_bad = proven(trial)
                if ok:
                    plan = trial
                    report["kept"].append(opt)
                    if attempt:
                        proof.kept_on_second_try(opt, worst, warn=False)
                    break
                worst[str(attempt)] = n_bad
            if opt not in report["kept"]:
                report["dropped"][opt] = worst
        return proof.finish(plan, is_int=lambda k: k in ("ln_flags", "attn_kb"), left_on="torch's own ops", per="pair")

    def plan_forward_against_module(self, module_forward, x, others) -> Optional[dict]:
        """Forward-only proof for the no-grad form.  -> the plan (installed), or None (module path)."""
        with torch.no_grad():
            y_ref = module_forward(x, others).detach()
            same = lambda plan: self._forward_same(plan, x, others, y_ref)  # noqa: E731

            plan = self.base_plan()
            if not same(plan) and not same(plan):
                self.plan_report = dict(usable=False)
                return None
            flags = next((f for f in LN_VARIANTS if self._ln_stats_match(x, f)), None)
            kept = []
            for opt in KERNEL_OPTS:
                if opt == "attn":
                    if others.get("attention_mask") is None:
                        continue
                    ok = False
                    for kb in key_block_candidates(ops.attn_key_block_guess(self.hd, int(x.shape[1]))):
                        trial = dict(plan, attn=True, attn_kb=kb)
                        ok = attention_forward_same(self, same, trial, runs=2)
                        if ok:
                            break
                elif flags is not None:
                    trial = dict(plan, **{opt: True, "ln_flags": flags})
                    ok = same(trial) and same(trial)
                else:
                    continue
                if ok:
                    plan = trial
                    kept.append(opt)
            self.set_plan(plan)
            self.plan_report = dict(usable=True, kept=kept, plan={k: (int(v) if k in ("ln_flags", "attn_kb") else bool(v)) for k, v in plan.items()})
        return plan
