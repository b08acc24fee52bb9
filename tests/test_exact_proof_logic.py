"""CPU pin of the PROOF POLICY of `exact_rounding`: which trial plans `plan_against_module` / `plan_forward_against_module` of
ExactLlamaBlock and ExactOPTBlock run, on which minibatch, in which order, and what they keep, drop, skip, report and warn about.

The real methods run on objects made with `object.__new__`; the device work is replaced through the seams the classes expose
(`_run_once`, `_forward_impl`, `_streamk_found`, `_attn_verify` / `_attn_diffs`) and three stubbed ops (`mse_loss_fwd_bwd`,
`rmsnorm_fwd_exact`, `layernorm_fwd_exact`).  A stubbed `_run_once` returns the module path's own result with a SCRIPTED number of
flipped values for (trial plan, minibatch, how often that pair was seen), so every branch of the acceptance rule can be driven.

Every case fixes, as literals read off the code before the rule moved into auto_round_amd/exact_proof.py:
  trials       each trial run as "<plan, as its difference from base_plan()>@<minibatch index>"
  plan         what the method returned, `installed` what `set_plan` left on the object
  report       the whole `plan_report` (its `plan` entry written on one line, values as `repr` prints them)
  warnings     every warning raised
  module_runs  (minibatch, every `_dw_accum` flag clear at that point) of each reference run; `accum_clear`: the flags after the proof
The differences between the two families (who gets a second pair, the base form's retry, one or two forward runs) are the families'
own behaviour and are pinned as they are."""
import types
import warnings

import pytest
import torch

ZERO4 = dict(out=0, dq=0, dk=0, dv=0)
S, H = 16, 8


class LlamaDecoderLayer:        # (only its name is used: the warnings print `type(self.block).__name__`)
    pass


class OPTDecoderLayer:
    pass


def _flip(t, n):
    """`t` with its first n values changed in one bit"""
    out = t.clone()
    if n:
        out.view(-1).view(torch.int16)[:n] ^= 1
    return out


class Harness:
    """One exact-block object over a fake arena, its seams scripted.

    script(d, mb, seen) -> differing values of the trial whose plan differs from the base plan by `d` (a dict), on minibatch `mb`, the
    `seen`-th time that pair runs (-1: the run raises RuntimeError); direct(d) -> what the attention verify run adds to `_attn_diffs`."""

    def __init__(self, family, mp, *, script=None, direct=None, mask=True, qk_norm=None, small=(), rms_ok=(False, True), ln_ok=(0,),
                 sk=None, wq_fresh=True):
        from auto_round_amd import ops

        self.script = script or (lambda d, mb, seen: 0)
        self.direct = direct or (lambda d: ZERO4)
        g = torch.Generator().manual_seed(0)
        self.xs = [torch.randn(1, S, H, generator=g).to(torch.bfloat16) for _ in range(2)]
        self.others = dict(attention_mask=torch.zeros(1, 1, S, S, dtype=torch.bfloat16) if mask else None)
        self.w = torch.full((H,), 2.0, dtype=torch.bfloat16, requires_grad=True)
        self.trials, self.module_runs, self.loss_calls, self.seen = [], [], [], {}
        self.arena = types.SimpleNamespace(wq_fresh=wq_fresh, dWq=torch.zeros(4, dtype=torch.bfloat16), qdq_calls=0,
                                           layers=[types.SimpleNamespace(_dw_accum=[True]) for _ in range(3)])
        self.arena.qdq_forward = lambda: setattr(self.arena, "qdq_calls", self.arena.qdq_calls + 1)
        if family == "llama":
            from auto_round_amd.exact_block import ExactLlamaBlock as cls

            keys, block, hd = "qkvogud", LlamaDecoderLayer(), 128
        else:
            from auto_round_amd.exact_opt_block import ExactOPTBlock as cls

            keys, block, hd = ("q", "k", "v", "o", "f1", "f2"), OPTDecoderLayer(), 64
        self.base = cls.base_plan()
        eb = self.eb = object.__new__(cls)
        eb.block, eb.arenas, eb.arena, eb.hd, eb.H, eb.dtype, eb.qk_norm = block, [self.arena], self.arena, hd, H, torch.bfloat16, qk_norm
        eb.layers = {k: types.SimpleNamespace(weight_q=torch.empty((1024, 1024) if k in small else (4096, 4096), dtype=torch.bfloat16, device="meta"))
                     for k in keys}
        eb.w1, eb.eps1 = torch.ones(H, dtype=torch.bfloat16), 1e-6
        eb.n1 = torch.nn.LayerNorm(H).to(torch.bfloat16)
        eb._tnx, eb._last_sk, eb.plan_report = {}, {}, None
        eb._attn_verify, eb._attn_diffs = False, {}
        eb.plan = cls.base_plan()
        eb._run_once = self._run_once
        eb._forward_impl = self._forward_impl
        eb._streamk_found = lambda key: (sk or {}).get(key)

        def rms(x2d, w, eps, rsqrt_f32=False, **kw):
            if rsqrt_f32 not in rms_ok:
                return None
            return None, torch.rsqrt(x2d.float().pow(2).mean(-1, keepdim=True) + eps).view(-1)

        def ln(x2d, w, b, eps, flags=0, want_stats=False):
            if flags not in ln_ok:
                return None
            y, mean, rstd = torch.ops.aten.native_layer_norm(x2d.float(), [H], w.float(), b.float(), eps)
            return y.to(x2d.dtype), mean.view(-1), rstd.view(-1)

        def mse(pred, ref, dpred=None, loss_accum=None, accum_scale=None, grad_scale=None):
            self.loss_calls.append((accum_scale, grad_scale))
            dpred.fill_(1.0)

        mp.setattr(ops, "rmsnorm_fwd_exact", rms)
        mp.setattr(ops, "layernorm_fwd_exact", ln)
        mp.setattr(ops, "mse_loss_fwd_bwd", mse)

    # -- what the block object sees ---------------------------------------------------------------------------------------
    def mb_of(self, x):
        return [t.data_ptr() for t in self.xs].index(x.data_ptr())

    def delta(self, plan):
        return {k: v for k, v in plan.items() if self.base.get(k) != v}

    @staticmethod
    def name(d):
        return ",".join(k if v is True else f"{k}={v}" for k, v in sorted(d.items()))

    def module_forward(self, x, others):
        self.module_runs.append((self.mb_of(x), not any(l._dw_accum[0] for l in self.arena.layers)))
        return x * self.w

    def _scripted(self, x, tag):
        d = self.delta(self.eb.plan)
        mb = self.mb_of(x)
        seen = self.seen.get((self.name(d), mb), 0)
        self.seen[(self.name(d), mb)] = seen + 1
        self.trials.append(f"{self.name(d)}@{mb}" if tag else self.name(d))
        if self.eb._attn_verify:
            for k, v in self.direct(d).items():
                self.eb._attn_diffs[k] = self.eb._attn_diffs.get(k, 0) + v
        n = self.script(d, mb, seen)
        if n < 0:
            raise RuntimeError("refused")
        return _flip((x * self.w).detach(), n)

    def _run_once(self, x, others, dpred):
        for l in self.arena.layers:
            l._dw_accum[0] = True
        return self._scripted(x, True), [self.arena.dWq.clone()]

    def _forward_impl(self, x, others, ctx):
        assert ctx is None
        return self._scripted(x, False)

    # -- the two proofs ---------------------------------------------------------------------------------------------------
    def _result(self, plan, caught, **more):
        report = dict(self.eb.plan_report)
        if "plan" in report:        # one line, and with each value's type (True == 1 would hide an int / bool slip)
            report["plan"] = " ".join(f"{k}={v!r}" for k, v in report["plan"].items())
        return dict(trials=self.trials, plan=None if plan is None else self.name(self.delta(plan)), installed=self.name(self.delta(self.eb.plan)),
                    report=report, warnings=[str(w.message) for w in caught], **more)

    def prove(self, want=None, second=True):
        x0, x1 = self.xs
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            plan = self.eb.plan_against_module(self.module_forward, x0, self.others, torch.zeros_like(x0), want=want,
                                               second=(x1, self.others, torch.zeros_like(x1)) if second else None)
        assert self.loss_calls == [(1.0, 1000.0)] * len(self.module_runs)
        return self._result(plan, caught, module_runs=self.module_runs, accum_clear=not any(l._dw_accum[0] for l in self.arena.layers),
                            qdq_calls=self.arena.qdq_calls)

    def prove_forward(self):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            plan = self.eb.plan_forward_against_module(self.module_forward, self.xs[0], self.others)
        return self._result(plan, caught)


ST = types.SimpleNamespace(grid=256, wgm=8, depth=32, n_dp=640, two_part_tiles=256)


def _is(d, **kv):
    """the trial's plan differs from the base plan in at least these values"""
    return all(d.get(k) == v for k, v in kv.items())


# ---- cases: name -> function(monkeypatch) -> result -----------------------------------------------------------------------------------
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


# -- Llama, forward + backward
@case
def llama_all_pass(mp):
    # (o_proj below 256 output tiles; the arena's weights not yet fake-quantised)
    return Harness("llama", mp, small=("o",), wq_fresh=False, sk=dict(d=[ST])).prove()


@case
def llama_all_pass_qk_norm_one_minibatch(mp):
    return Harness("llama", mp, qk_norm=(None, None, 1e-6)).prove(want=("norm1", "qknorm", "rope"), second=False)


@case
def llama_want_filter_reaches_default_skip(mp):
    return Harness("llama", mp).prove(want=("rope", "merged_gu", "tn_d"))


@case
def llama_base_differs(mp):
    return Harness("llama", mp, script=lambda d, mb, seen: 0 if d else 3).prove()


@case
def llama_base_differs_on_second_minibatch(mp):
    return Harness("llama", mp, script=lambda d, mb, seen: 5 if (not d and mb == 1) else 0).prove()


@case
def llama_one_of_two_is_dropped(mp):
    return Harness("llama", mp, script=lambda d, mb, seen: 7 if (_is(d, rope=True) and mb == 1) else 0).prove(want=("rope", "swiglu"))


@case
def llama_kernel_option_kept_on_second_pair(mp):
    return Harness("llama", mp, script=lambda d, mb, seen: 2 if (_is(d, rope=True) and mb == 0 and seen == 0) else 0).prove(want=("rope",))


@case
def llama_dw_option_gets_no_second_pair(mp):
    return Harness("llama", mp, script=lambda d, mb, seen: 4 if "dw_d" in d and seen == 0 else 0).prove(want=("dw_d",))


@case
def llama_dw_variants_and_streamk(mp):
    def script(d, mb, seen):
        if "dw_d" in d and d["dw_d"] in (1, 2):
            return 6
        if "dw_gu" in d and d["dw_gu"] != -1:
            return 9 if mb == 0 else 0
        return 0

    # dw_qkv: one pass matches; dw_gu: only the stream-K form matches, its structure found (gate: stream-K, up: one pass);
    # dw_d: three K slices; dw_o: every slicing differs, the stream-K form matches but no structure was found
    def script_o(d, mb, seen):
        if "dw_o" in d and d["dw_o"] != -1:
            return 1
        return script(d, mb, seen)

    return Harness("llama", mp, script=script_o, sk=dict(gu=[ST, None])).prove(want=("dw_qkv", "dw_gu", "dw_q", "dw_g", "dw_o", "dw_d"))


@case
def llama_swiglu_second_variant(mp):
    return Harness("llama", mp, script=lambda d, mb, seen: 3 if (_is(d, swiglu=True) and "swiglu_contract" not in d) else 0).prove(want=("swiglu",))


@case
def llama_norms_take_the_rsqrt_form_whose_statistics_match(mp):
    return Harness("llama", mp, qk_norm=(None, None, 1e-6), rms_ok=(True,)).prove(want=("norm1", "norm2", "qknorm"))


@case
def llama_norms_try_the_second_form_when_the_first_differs(mp):
    return Harness("llama", mp, script=lambda d, mb, seen: 2 if (_is(d, norm1=True) and "norm_rsqrt_f32" not in d) else 0).prove(want=("norm1", "norm2"))


@case
def llama_norm_statistics_differ(mp):
    return Harness("llama", mp, qk_norm=(None, None, 1e-6), rms_ok=()).prove(want=("norm1", "norm2", "qknorm", "rope"))


@case
def llama_attention_key_blocks(mp):
    # the guess differs in the block output, 64 has equal block bits but a differing dq, 16 matches
    return Harness("llama", mp, script=lambda d, mb, seen: 11 if _is(d, attn=True) and "attn_kb" not in d else 0,
                   direct=lambda d: dict(ZERO4, dq=2) if d.get("attn_kb") == 64 else ZERO4).prove(want=("attn",))


@case
def llama_attention_direct_diff_missing(mp):
    return Harness("llama", mp, direct=lambda d: dict(out=0, dq=0, dk=0)).prove(want=("attn", "rope"))


@case
def llama_attention_without_a_mask(mp):
    return Harness("llama", mp, mask=False).prove(want=("attn",))


@case
def llama_refusal(mp):
    return Harness("llama", mp, script=lambda d, mb, seen: -1 if _is(d, rope=True) else 0).prove(want=("rope", "swiglu"))


# -- OPT, forward + backward
@case
def opt_all_pass(mp):
    return Harness("opt", mp, wq_fresh=False).prove()


@case
def opt_ln_flags_first_matching(mp):
    return Harness("opt", mp, ln_ok=(2, 3)).prove(want=("ln1", "ln2"))


@case
def opt_no_layernorm_form_matches(mp):
    return Harness("opt", mp, ln_ok=()).prove()


@case
def opt_base_kept_on_second_pair(mp):
    return Harness("opt", mp, script=lambda d, mb, seen: 4 if (not d and mb == 1 and seen == 0) else 0).prove(want=("ln1",))


@case
def opt_base_differs_twice(mp):
    return Harness("opt", mp, script=lambda d, mb, seen: 0 if d else 3 + seen).prove()


@case
def opt_one_of_two_is_dropped(mp):
    return Harness("opt", mp, script=lambda d, mb, seen: 7 if (_is(d, ln1=True) and mb == 1) else 0).prove(want=("ln1", "ln2"))


@case
def opt_kernel_option_retries_only_its_first_variant(mp):
    # every key block differs once; the retry of the guess matches
    return Harness("opt", mp, script=lambda d, mb, seen: 5 if (_is(d, attn=True) and seen == 0) else 0).prove(want=("attn",))


@case
def opt_attention_key_blocks(mp):
    return Harness("opt", mp, script=lambda d, mb, seen: 11 if _is(d, attn=True) and "attn_kb" not in d else 0,
                   direct=lambda d: dict(ZERO4, dv=1) if d.get("attn_kb") == 32 else ZERO4).prove(want=("attn",))


@case
def opt_attention_direct_diff_missing(mp):
    return Harness("opt", mp, direct=lambda d: dict(out=0, dq=0, dk=0)).prove(want=("attn",))


@case
def opt_attention_without_a_mask(mp):
    return Harness("opt", mp, mask=False).prove(want=("attn", "merged_qkv"))


@case
def opt_gemm_options_get_two_attempts(mp):
    def script(d, mb, seen):
        if _is(d, merged_qkv=True) and "dw_qkv" not in d:
            return 2 if seen == 0 and mb == 0 else 0
        return 8 if _is(d, dw_qkv=True) else 0

    return Harness("opt", mp, script=script).prove(want=("merged_qkv", "dw_qkv"))


@case
def opt_refusal(mp):
    return Harness("opt", mp, script=lambda d, mb, seen: -1 if _is(d, ln2=True) else 0).prove(want=("ln2", "dw_qkv"))


# -- forward-only
@case
def llama_forward_all_pass(mp):
    return Harness("llama", mp, qk_norm=(None, None, 1e-6)).prove_forward()


@case
def llama_forward_base_differs(mp):
    return Harness("llama", mp, script=lambda d, mb, seen: 0 if d else 1).prove_forward()


@case
def llama_forward_attention_and_unproven_norms(mp):
    # the row statistics differ: no norm option; the guess has a differing attention output, 64 matches
    return Harness("llama", mp, qk_norm=(None, None, 1e-6), rms_ok=(),
                   direct=lambda d: dict(out=0 if d.get("attn_kb") == 64 else 3)).prove_forward()


@case
def llama_forward_attention_never_compared(mp):
    return Harness("llama", mp, direct=lambda d: {}).prove_forward()


@case
def llama_forward_without_a_mask_and_a_refusal(mp):
    return Harness("llama", mp, mask=False, script=lambda d, mb, seen: -1 if _is(d, swiglu=True) else 0).prove_forward()


@case
def opt_forward_all_pass(mp):
    return Harness("opt", mp).prove_forward()


@case
def opt_forward_base_passes_on_its_second_run(mp):
    return Harness("opt", mp, script=lambda d, mb, seen: 1 if (not d and seen == 0) else 0, ln_ok=(1,)).prove_forward()


@case
def opt_forward_base_differs_twice(mp):
    return Harness("opt", mp, script=lambda d, mb, seen: 0 if d else 1).prove_forward()


@case
def opt_forward_second_run_differs(mp):
    return Harness("opt", mp, script=lambda d, mb, seen: 1 if (_is(d, ln1=True) and "ln2" not in d and seen == 1) else 0).prove_forward()


@case
def opt_forward_no_layernorm_form_and_attention_key_blocks(mp):
    return Harness("opt", mp, ln_ok=(), direct=lambda d: dict(out=0 if d.get("attn_kb") == 16 else 2)).prove_forward()


@case
def opt_forward_without_a_mask(mp):
    return Harness("opt", mp, mask=False).prove_forward()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_proof_runs_these_trials_and_reports_this(name, monkeypatch):
    got = CASES[name](monkeypatch)
    want = EXPECTED[name]
    for key in sorted(set(got) | set(want)):
        assert got.get(key) == want.get(key), (name, key)


# ---- the literals ------------------------------------------------------------------------------------------------------------------------
EXPECTED = {'llama_all_pass': {'trials': ['@0',
                               '@1',
                               'norm1@0',
                               'norm1@1',
                               'norm1,norm2@0',
                               'norm1,norm2@1',
                               'norm1,norm2,rope@0',
                               'norm1,norm2,rope@1',
                               'norm1,norm2,rope,swiglu@0',
                               'norm1,norm2,rope,swiglu@1',
                               'attn,norm1,norm2,rope,swiglu@0',
                               'attn,norm1,norm2,rope,swiglu@1',
                               'attn,norm1,norm2,rope,swiglu,tn_o@0',
                               'attn,norm1,norm2,rope,swiglu,tn_o@1',
                               'attn,norm1,norm2,rope,swiglu,tn_g,tn_o@0',
                               'attn,norm1,norm2,rope,swiglu,tn_g,tn_o@1',
                               'attn,norm1,norm2,rope,swiglu,tn_g,tn_o,tn_u@0',
                               'attn,norm1,norm2,rope,swiglu,tn_g,tn_o,tn_u@1',
                               'attn,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u@0',
                               'attn,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u@1',
                               'attn,dw_qkv=1,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u@0',
                               'attn,dw_qkv=1,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u@1',
                               'attn,dw_gu=1,dw_qkv=1,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u@0',
                               'attn,dw_gu=1,dw_qkv=1,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u@1',
                               'attn,dw_d=1,dw_gu=1,dw_qkv=1,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u@0',
                               'attn,dw_d=1,dw_gu=1,dw_qkv=1,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u@1'],
                    'plan': 'attn,dw_d=1,dw_gu=1,dw_qkv=1,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u',
                    'installed': 'attn,dw_d=1,dw_gu=1,dw_qkv=1,norm1,norm2,rope,swiglu,tn_d,tn_g,tn_o,tn_u',
                    'report': {'errors': {},
                               'tried': ['norm1', 'norm2', 'rope', 'swiglu', 'attn', 'tn_o', 'tn_g', 'tn_u', 'tn_d', 'dw_qkv', 'dw_gu', 'dw_d'],
                               'kept': ['norm1', 'norm2', 'rope', 'swiglu', 'attn', 'tn_o', 'tn_g', 'tn_u', 'tn_d', 'dw_qkv', 'dw_gu', 'dw_d'],
                               'skipped': {'dw_q': 'covered by the merged weight-gradient GEMM',
                                           'dw_k': 'covered by the merged weight-gradient GEMM',
                                           'dw_v': 'covered by the merged weight-gradient GEMM',
                                           'dw_o': 'fewer than 256 output tiles: the library GEMM is the faster one',
                                           'dw_g': 'covered by the merged weight-gradient GEMM',
                                           'dw_u': 'covered by the merged weight-gradient GEMM'},
                               'dropped': {},
                               'minibatches': 2,
                               'attn_direct': [{'out': 0, 'dq': 0, 'dk': 0, 'dv': 0}],
                               'usable': True,
                               'plan': 'norm1=True norm2=True qknorm=False rope=True swiglu=True attn=True tn_o=True tn_g=True tn_u=True tn_d=True '
                                       'dw_qkv=1 dw_gu=1 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 dw_d=1 merged_qkv=False merged_gu=False '
                                       'swiglu_contract=True norm_rsqrt_f32=False attn_kb=0'},
                    'warnings': [],
                    'module_runs': [(0, True), (1, True)],
                    'accum_clear': True,
                    'qdq_calls': 1},
 'llama_all_pass_qk_norm_one_minibatch': {'trials': ['@0',
                                                     '@0',
                                                     'norm1@0',
                                                     'norm1@0',
                                                     'norm1,qknorm@0',
                                                     'norm1,qknorm@0',
                                                     'norm1,qknorm,rope@0',
                                                     'norm1,qknorm,rope@0'],
                                          'plan': 'norm1,qknorm,rope',
                                          'installed': 'norm1,qknorm,rope',
                                          'report': {'errors': {},
                                                     'tried': ['norm1', 'qknorm', 'rope'],
                                                     'kept': ['norm1', 'qknorm', 'rope'],
                                                     'skipped': {},
                                                     'dropped': {},
                                                     'minibatches': 1,
                                                     'usable': True,
                                                     'plan': 'norm1=True norm2=False qknorm=True rope=True swiglu=False attn=False tn_o=False '
                                                             'tn_g=False tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 '
                                                             'dw_u=0 dw_d=0 merged_qkv=False merged_gu=False swiglu_contract=True '
                                                             'norm_rsqrt_f32=False attn_kb=0'},
                                          'warnings': [],
                                          'module_runs': [(0, True)],
                                          'accum_clear': True,
                                          'qdq_calls': 0},
 'llama_attention_direct_diff_missing': {'trials': ['@0',
                                                    '@1',
                                                    'rope@0',
                                                    'rope@1',
                                                    'attn,rope@0',
                                                    'attn,rope@1',
                                                    'attn,attn_kb=64,rope@0',
                                                    'attn,attn_kb=64,rope@1',
                                                    'attn,attn_kb=16,rope@0',
                                                    'attn,attn_kb=16,rope@1',
                                                    'attn,rope@0',
                                                    'attn,rope@1',
                                                    'attn,attn_kb=64,rope@0',
                                                    'attn,attn_kb=64,rope@1',
                                                    'attn,attn_kb=16,rope@0',
                                                    'attn,attn_kb=16,rope@1'],
                                         'plan': 'rope',
                                         'installed': 'rope',
                                         'report': {'errors': {},
                                                    'tried': ['rope', 'attn'],
                                                    'kept': ['rope'],
                                                    'skipped': {},
                                                    'dropped': {'attn': {'0': -1, '1': -1, '2': -1}},
                                                    'minibatches': 2,
                                                    'attn_direct': [{'out': 0, 'dq': 0, 'dk': 0},
                                                                    {'out': 0, 'dq': 0, 'dk': 0},
                                                                    {'out': 0, 'dq': 0, 'dk': 0},
                                                                    {'out': 0, 'dq': 0, 'dk': 0},
                                                                    {'out': 0, 'dq': 0, 'dk': 0},
                                                                    {'out': 0, 'dq': 0, 'dk': 0}],
                                                    'usable': True,
                                                    'plan': 'norm1=False norm2=False qknorm=False rope=True swiglu=False attn=False tn_o=False '
                                                            'tn_g=False tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 '
                                                            'dw_u=0 dw_d=0 merged_qkv=False merged_gu=False swiglu_contract=True '
                                                            'norm_rsqrt_f32=False attn_kb=0'},
                                         'warnings': ['exact_rounding: LlamaDecoderLayer: not bit-equal to the module path on this stack and left on '
                                                      "the module path's own form (slower): {'attn': {'0': -1, '1': -1, '2': -1}} (differing values "
                                                      'per tried form)'],
                                         'module_runs': [(0, True), (1, True)],
                                         'accum_clear': True,
                                         'qdq_calls': 0},
 'llama_attention_key_blocks': {'trials': ['@0', '@1', 'attn@0', 'attn,attn_kb=64@0', 'attn,attn_kb=64@1', 'attn,attn_kb=16@0', 'attn,attn_kb=16@1'],
                                'plan': 'attn,attn_kb=16',
                                'installed': 'attn,attn_kb=16',
                                'report': {'errors': {},
                                           'tried': ['attn'],
                                           'kept': ['attn'],
                                           'skipped': {},
                                           'dropped': {},
                                           'minibatches': 2,
                                           'attn_direct': [{'out': 0, 'dq': 0, 'dk': 0, 'dv': 0},
                                                           {'out': 0, 'dq': 4, 'dk': 0, 'dv': 0},
                                                           {'out': 0, 'dq': 0, 'dk': 0, 'dv': 0}],
                                           'usable': True,
                                           'plan': 'norm1=False norm2=False qknorm=False rope=False swiglu=False attn=True tn_o=False tn_g=False '
                                                   'tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 dw_d=0 '
                                                   'merged_qkv=False merged_gu=False swiglu_contract=True norm_rsqrt_f32=False attn_kb=16'},
                                'warnings': [],
                                'module_runs': [(0, True), (1, True)],
                                'accum_clear': True,
                                'qdq_calls': 0},
 'llama_attention_without_a_mask': {'trials': ['@0', '@1'],
                                    'plan': '',
                                    'installed': '',
                                    'report': {'errors': {},
                                               'tried': [],
                                               'kept': [],
                                               'skipped': {'attn': 'no additive attention mask: the call is not the one the kernel restates'},
                                               'dropped': {},
                                               'minibatches': 2,
                                               'usable': True,
                                               'plan': 'norm1=False norm2=False qknorm=False rope=False swiglu=False attn=False tn_o=False '
                                                       'tn_g=False tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 '
                                                       'dw_d=0 merged_qkv=False merged_gu=False swiglu_contract=True norm_rsqrt_f32=False attn_kb=0'},
                                    'warnings': [],
                                    'module_runs': [(0, True), (1, True)],
                                    'accum_clear': True,
                                    'qdq_calls': 0},
 'llama_base_differs': {'trials': ['@0'],
                        'plan': None,
                        'installed': '',
                        'report': {'errors': {},
                                   'tried': [],
                                   'kept': [],
                                   'skipped': {},
                                   'dropped': {},
                                   'minibatches': 2,
                                   'usable': False,
                                   'base_mismatches': 3},
                        'warnings': ["exact_rounding: even with every segment on torch's own ops LlamaDecoderLayer differs from the module path (3 "
                                     'values); blocks of this kind keep the module path'],
                        'module_runs': [(0, True), (1, True)],
                        'accum_clear': True,
                        'qdq_calls': 0},
 'llama_base_differs_on_second_minibatch': {'trials': ['@0', '@1'],
                                            'plan': None,
                                            'installed': '',
                                            'report': {'errors': {},
                                                       'tried': [],
                                                       'kept': [],
                                                       'skipped': {},
                                                       'dropped': {},
                                                       'minibatches': 2,
                                                       'usable': False,
                                                       'base_mismatches': 5},
                                            'warnings': ["exact_rounding: even with every segment on torch's own ops LlamaDecoderLayer differs from "
                                                         'the module path (5 values); blocks of this kind keep the module path'],
                                            'module_runs': [(0, True), (1, True)],
                                            'accum_clear': True,
                                            'qdq_calls': 0},
 'llama_dw_option_gets_no_second_pair': {'trials': ['@0', '@1', 'dw_d=1@0', 'dw_d=2@0', 'dw_d=3@0', 'dw_d=4@0', 'dw_d=-1@0'],
                                         'plan': '',
                                         'installed': '',
                                         'report': {'errors': {},
                                                    'tried': ['dw_d'],
                                                    'kept': [],
                                                    'skipped': {},
                                                    'dropped': {'dw_d': {'1': 4, '2': 4, '3': 4, '4': 4, '-1': 4}},
                                                    'minibatches': 2,
                                                    'usable': True,
                                                    'plan': 'norm1=False norm2=False qknorm=False rope=False swiglu=False attn=False tn_o=False '
                                                            'tn_g=False tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 '
                                                            'dw_u=0 dw_d=0 merged_qkv=False merged_gu=False swiglu_contract=True '
                                                            'norm_rsqrt_f32=False attn_kb=0'},
                                         'warnings': ['exact_rounding: LlamaDecoderLayer: not bit-equal to the module path on this stack and left on '
                                                      "the module path's own form (slower): {'dw_d': {'1': 4, '2': 4, '3': 4, '4': 4, '-1': 4}} "
                                                      '(differing values per tried form)'],
                                         'module_runs': [(0, True), (1, True)],
                                         'accum_clear': True,
                                         'qdq_calls': 0},
 'llama_dw_variants_and_streamk': {'trials': ['@0',
                                              '@1',
                                              'dw_qkv=1@0',
                                              'dw_qkv=1@1',
                                              'dw_gu=1,dw_qkv=1@0',
                                              'dw_gu=2,dw_qkv=1@0',
                                              'dw_gu=3,dw_qkv=1@0',
                                              'dw_gu=4,dw_qkv=1@0',
                                              'dw_gu=-1,dw_qkv=1@0',
                                              'dw_gu=-1,dw_qkv=1@1',
                                              'dw_gu=-1,dw_o=1,dw_qkv=1@0',
                                              'dw_gu=-1,dw_o=2,dw_qkv=1@0',
                                              'dw_gu=-1,dw_o=3,dw_qkv=1@0',
                                              'dw_gu=-1,dw_o=4,dw_qkv=1@0',
                                              'dw_gu=-1,dw_o=-1,dw_qkv=1@0',
                                              'dw_gu=-1,dw_o=-1,dw_qkv=1@1',
                                              'dw_d=1,dw_gu=-1,dw_qkv=1@0',
                                              'dw_d=2,dw_gu=-1,dw_qkv=1@0',
                                              'dw_d=3,dw_gu=-1,dw_qkv=1@0',
                                              'dw_d=3,dw_gu=-1,dw_qkv=1@1'],
                                   'plan': 'dw_d=3,dw_gu=-1,dw_qkv=1',
                                   'installed': 'dw_d=3,dw_gu=-1,dw_qkv=1',
                                   'report': {'errors': {},
                                              'tried': ['dw_qkv', 'dw_gu', 'dw_o', 'dw_d'],
                                              'kept': ['dw_qkv', 'dw_gu', 'dw_d'],
                                              'skipped': {'dw_q': 'covered by the merged weight-gradient GEMM',
                                                          'dw_g': 'covered by the merged weight-gradient GEMM'},
                                              'dropped': {'dw_o': {'1': 1,
                                                                   '2': 1,
                                                                   '3': 1,
                                                                   '4': 1,
                                                                   'STREAMK': "no structure reproduces the library's result"}},
                                              'minibatches': 2,
                                              'streamk': {'dw_gu': [{'grid': 256,
                                                                     'wgm': 8,
                                                                     'depth': 32,
                                                                     'one_pass_tiles': 640,
                                                                     'two_part_tiles': 256},
                                                                    {'one_pass': True}]},
                                              'usable': True,
                                              'plan': 'norm1=False norm2=False qknorm=False rope=False swiglu=False attn=False tn_o=False tn_g=False '
                                                      'tn_u=False tn_d=False dw_qkv=1 dw_gu=-1 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 dw_d=3 '
                                                      'merged_qkv=False merged_gu=False swiglu_contract=True norm_rsqrt_f32=False attn_kb=0'},
                                   'warnings': ['exact_rounding: LlamaDecoderLayer: not bit-equal to the module path on this stack and left on the '
                                                "module path's own form (slower): {'dw_o': {'1': 1, '2': 1, '3': 1, '4': 1, 'STREAMK': "
                                                '"no structure reproduces the library\'s result"}} (differing values per tried form)'],
                                   'module_runs': [(0, True), (1, True)],
                                   'accum_clear': True,
                                   'qdq_calls': 0},
 'llama_forward_all_pass': {'trials': ['',
                                       'norm1',
                                       'norm1,norm2',
                                       'norm1,norm2,qknorm',
                                       'norm1,norm2,qknorm,rope',
                                       'norm1,norm2,qknorm,rope,swiglu',
                                       'attn,norm1,norm2,qknorm,rope,swiglu'],
                            'plan': 'attn,norm1,norm2,qknorm,rope,swiglu',
                            'installed': 'attn,norm1,norm2,qknorm,rope,swiglu',
                            'report': {'usable': True,
                                       'kept': ['norm1', 'norm2', 'qknorm', 'rope', 'swiglu', 'attn'],
                                       'plan': 'norm1=True norm2=True qknorm=True rope=True swiglu=True attn=True attn_kb=0'},
                            'warnings': []},
 'llama_forward_attention_and_unproven_norms': {'trials': ['', 'rope', 'rope,swiglu', 'attn,rope,swiglu', 'attn,attn_kb=64,rope,swiglu'],
                                                'plan': 'attn,attn_kb=64,rope,swiglu',
                                                'installed': 'attn,attn_kb=64,rope,swiglu',
                                                'report': {'usable': True,
                                                           'kept': ['rope', 'swiglu', 'attn'],
                                                           'plan': 'norm1=False norm2=False qknorm=False rope=True swiglu=True attn=True attn_kb=64'},
                                                'warnings': []},
 'llama_forward_attention_never_compared': {'trials': ['',
                                                       'norm1',
                                                       'norm1,norm2',
                                                       'norm1,norm2,rope',
                                                       'norm1,norm2,rope,swiglu',
                                                       'attn,norm1,norm2,rope,swiglu',
                                                       'attn,attn_kb=64,norm1,norm2,rope,swiglu',
                                                       'attn,attn_kb=16,norm1,norm2,rope,swiglu'],
                                            'plan': 'norm1,norm2,rope,swiglu',
                                            'installed': 'norm1,norm2,rope,swiglu',
                                            'report': {'usable': True,
                                                       'kept': ['norm1', 'norm2', 'rope', 'swiglu'],
                                                       'plan': 'norm1=True norm2=True qknorm=False rope=True swiglu=True attn=False attn_kb=0'},
                                            'warnings': []},
 'llama_forward_base_differs': {'trials': [''], 'plan': None, 'installed': '', 'report': {'usable': False}, 'warnings': []},
 'llama_forward_without_a_mask_and_a_refusal': {'trials': ['', 'norm1', 'norm1,norm2', 'norm1,norm2,rope', 'norm1,norm2,rope,swiglu'],
                                                'plan': 'norm1,norm2,rope',
                                                'installed': 'norm1,norm2,rope',
                                                'report': {'usable': True,
                                                           'kept': ['norm1', 'norm2', 'rope'],
                                                           'plan': 'norm1=True norm2=True qknorm=False rope=True swiglu=False attn=False attn_kb=0'},
                                                'warnings': []},
 'llama_kernel_option_kept_on_second_pair': {'trials': ['@0', '@1', 'rope@0', 'rope@0', 'rope@1'],
                                             'plan': 'rope',
                                             'installed': 'rope',
                                             'report': {'errors': {},
                                                        'tried': ['rope'],
                                                        'kept': ['rope'],
                                                        'skipped': {},
                                                        'dropped': {},
                                                        'minibatches': 2,
                                                        'kept_on_second_try': ['rope'],
                                                        'usable': True,
                                                        'plan': 'norm1=False norm2=False qknorm=False rope=True swiglu=False attn=False tn_o=False '
                                                                'tn_g=False tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 '
                                                                'dw_g=0 dw_u=0 dw_d=0 merged_qkv=False merged_gu=False swiglu_contract=True '
                                                                'norm_rsqrt_f32=False attn_kb=0'},
                                             'warnings': ['exact_rounding: option rope differed from the module path in its first pair of runs '
                                                          "({'0': 2}) and matched in the second pair -- kept; the library under the comparison is "
                                                          'not perfectly repeatable'],
                                             'module_runs': [(0, True), (1, True)],
                                             'accum_clear': True,
                                             'qdq_calls': 0},
 'llama_norm_statistics_differ': {'trials': ['@0', '@1', 'rope@0', 'rope@1'],
                                  'plan': 'rope',
                                  'installed': 'rope',
                                  'report': {'errors': {'norm1': "row statistics differ from torch's (rsqrt / reduction order)",
                                                        'norm2': "row statistics differ from torch's (rsqrt / reduction order)"},
                                             'tried': ['norm1', 'norm2', 'rope'],
                                             'kept': ['rope'],
                                             'skipped': {'qknorm': "the RMSNorm kernels did not reproduce torch's row statistics on this stack"},
                                             'dropped': {'norm1': {}, 'norm2': {}},
                                             'minibatches': 2,
                                             'usable': True,
                                             'plan': 'norm1=False norm2=False qknorm=False rope=True swiglu=False attn=False tn_o=False tn_g=False '
                                                     'tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 dw_d=0 '
                                                     'merged_qkv=False merged_gu=False swiglu_contract=True norm_rsqrt_f32=False attn_kb=0'},
                                  'warnings': ['exact_rounding: LlamaDecoderLayer: not bit-equal to the module path on this stack and left on the '
                                               "module path's own form (slower): {'norm1': {}, 'norm2': {}} (differing values per tried form)"],
                                  'module_runs': [(0, True), (1, True)],
                                  'accum_clear': True,
                                  'qdq_calls': 0},
 'llama_norms_take_the_rsqrt_form_whose_statistics_match': {'trials': ['@0',
                                                                       '@1',
                                                                       'norm1,norm_rsqrt_f32@0',
                                                                       'norm1,norm_rsqrt_f32@1',
                                                                       'norm1,norm2,norm_rsqrt_f32@0',
                                                                       'norm1,norm2,norm_rsqrt_f32@1',
                                                                       'norm1,norm2,norm_rsqrt_f32,qknorm@0',
                                                                       'norm1,norm2,norm_rsqrt_f32,qknorm@1'],
                                                            'plan': 'norm1,norm2,norm_rsqrt_f32,qknorm',
                                                            'installed': 'norm1,norm2,norm_rsqrt_f32,qknorm',
                                                            'report': {'errors': {},
                                                                       'tried': ['norm1', 'norm2', 'qknorm'],
                                                                       'kept': ['norm1', 'norm2', 'qknorm'],
                                                                       'skipped': {},
                                                                       'dropped': {},
                                                                       'minibatches': 2,
                                                                       'usable': True,
                                                                       'plan': 'norm1=True norm2=True qknorm=True rope=False swiglu=False attn=False '
                                                                               'tn_o=False tn_g=False tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 '
                                                                               'dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 dw_d=0 merged_qkv=False '
                                                                               'merged_gu=False swiglu_contract=True norm_rsqrt_f32=True attn_kb=0'},
                                                            'warnings': [],
                                                            'module_runs': [(0, True), (1, True)],
                                                            'accum_clear': True,
                                                            'qdq_calls': 0},
 'llama_norms_try_the_second_form_when_the_first_differs': {'trials': ['@0',
                                                                       '@1',
                                                                       'norm1@0',
                                                                       'norm1,norm_rsqrt_f32@0',
                                                                       'norm1,norm_rsqrt_f32@1',
                                                                       'norm1,norm2,norm_rsqrt_f32@0',
                                                                       'norm1,norm2,norm_rsqrt_f32@1'],
                                                            'plan': 'norm1,norm2,norm_rsqrt_f32',
                                                            'installed': 'norm1,norm2,norm_rsqrt_f32',
                                                            'report': {'errors': {},
                                                                       'tried': ['norm1', 'norm2'],
                                                                       'kept': ['norm1', 'norm2'],
                                                                       'skipped': {},
                                                                       'dropped': {},
                                                                       'minibatches': 2,
                                                                       'usable': True,
                                                                       'plan': 'norm1=True norm2=True qknorm=False rope=False swiglu=False '
                                                                               'attn=False tn_o=False tn_g=False tn_u=False tn_d=False dw_qkv=0 '
                                                                               'dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 dw_d=0 '
                                                                               'merged_qkv=False merged_gu=False swiglu_contract=True '
                                                                               'norm_rsqrt_f32=True attn_kb=0'},
                                                            'warnings': [],
                                                            'module_runs': [(0, True), (1, True)],
                                                            'accum_clear': True,
                                                            'qdq_calls': 0},
 'llama_one_of_two_is_dropped': {'trials': ['@0', '@1', 'rope@0', 'rope@1', 'rope@0', 'rope@1', 'swiglu@0', 'swiglu@1'],
                                 'plan': 'swiglu',
                                 'installed': 'swiglu',
                                 'report': {'errors': {},
                                            'tried': ['rope', 'swiglu'],
                                            'kept': ['swiglu'],
                                            'skipped': {},
                                            'dropped': {'rope': {'0': 7}},
                                            'minibatches': 2,
                                            'usable': True,
                                            'plan': 'norm1=False norm2=False qknorm=False rope=False swiglu=True attn=False tn_o=False tn_g=False '
                                                    'tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 dw_d=0 '
                                                    'merged_qkv=False merged_gu=False swiglu_contract=True norm_rsqrt_f32=False attn_kb=0'},
                                 'warnings': ['exact_rounding: LlamaDecoderLayer: not bit-equal to the module path on this stack and left on the '
                                              "module path's own form (slower): {'rope': {'0': 7}} (differing values per tried form)"],
                                 'module_runs': [(0, True), (1, True)],
                                 'accum_clear': True,
                                 'qdq_calls': 0},
 'llama_refusal': {'trials': ['@0', '@1', 'rope@0', 'rope@0', 'swiglu@0', 'swiglu@1'],
                   'plan': 'swiglu',
                   'installed': 'swiglu',
                   'report': {'errors': {'rope,swiglu_contract': "RuntimeError('refused')"},
                              'tried': ['rope', 'swiglu'],
                              'kept': ['swiglu'],
                              'skipped': {},
                              'dropped': {'rope': {'0': -1}},
                              'minibatches': 2,
                              'usable': True,
                              'plan': 'norm1=False norm2=False qknorm=False rope=False swiglu=True attn=False tn_o=False tn_g=False tn_u=False '
                                      'tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 dw_d=0 merged_qkv=False merged_gu=False '
                                      'swiglu_contract=True norm_rsqrt_f32=False attn_kb=0'},
                   'warnings': ["exact_rounding: LlamaDecoderLayer: not bit-equal to the module path on this stack and left on the module path's own "
                                "form (slower): {'rope': {'0': -1}} (differing values per tried form)"],
                   'module_runs': [(0, True), (1, True)],
                   'accum_clear': True,
                   'qdq_calls': 0},
 'llama_swiglu_second_variant': {'trials': ['@0', '@1', 'swiglu@0', 'swiglu,swiglu_contract=False@0', 'swiglu,swiglu_contract=False@1'],
                                 'plan': 'swiglu,swiglu_contract=False',
                                 'installed': 'swiglu,swiglu_contract=False',
                                 'report': {'errors': {},
                                            'tried': ['swiglu'],
                                            'kept': ['swiglu'],
                                            'skipped': {},
                                            'dropped': {},
                                            'minibatches': 2,
                                            'usable': True,
                                            'plan': 'norm1=False norm2=False qknorm=False rope=False swiglu=True attn=False tn_o=False tn_g=False '
                                                    'tn_u=False tn_d=False dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 dw_u=0 dw_d=0 '
                                                    'merged_qkv=False merged_gu=False swiglu_contract=False norm_rsqrt_f32=False attn_kb=0'},
                                 'warnings': [],
                                 'module_runs': [(0, True), (1, True)],
                                 'accum_clear': True,
                                 'qdq_calls': 0},
 'llama_want_filter_reaches_default_skip': {'trials': ['@0',
                                                       '@1',
                                                       'rope@0',
                                                       'rope@1',
                                                       'rope,tn_d@0',
                                                       'rope,tn_d@1',
                                                       'merged_gu,rope,tn_d@0',
                                                       'merged_gu,rope,tn_d@1'],
                                            'plan': 'merged_gu,rope,tn_d',
                                            'installed': 'merged_gu,rope,tn_d',
                                            'report': {'errors': {},
                                                       'tried': ['rope', 'tn_d', 'merged_gu'],
                                                       'kept': ['rope', 'tn_d', 'merged_gu'],
                                                       'skipped': {},
                                                       'dropped': {},
                                                       'minibatches': 2,
                                                       'usable': True,
                                                       'plan': 'norm1=False norm2=False qknorm=False rope=True swiglu=False attn=False tn_o=False '
                                                               'tn_g=False tn_u=False tn_d=True dw_qkv=0 dw_gu=0 dw_q=0 dw_k=0 dw_v=0 dw_o=0 dw_g=0 '
                                                               'dw_u=0 dw_d=0 merged_qkv=False merged_gu=True swiglu_contract=True '
                                                               'norm_rsqrt_f32=False attn_kb=0'},
                                            'warnings': [],
                                            'module_runs': [(0, True), (1, True)],
                                            'accum_clear': True,
                                            'qdq_calls': 0},
 'opt_all_pass': {'trials': ['@0',
                             '@1',
                             'ln1@0',
                             'ln1@1',
                             'ln1,ln2@0',
                             'ln1,ln2@1',
                             'attn,ln1,ln2@0',
                             'attn,ln1,ln2@1',
                             'attn,ln1,ln2,merged_qkv@0',
                             'attn,ln1,ln2,merged_qkv@1',
                             'attn,dw_qkv,ln1,ln2,merged_qkv@0',
                             'attn,dw_qkv,ln1,ln2,merged_qkv@1'],
                  'plan': 'attn,dw_qkv,ln1,ln2,merged_qkv',
                  'installed': 'attn,dw_qkv,ln1,ln2,merged_qkv',
                  'report': {'errors': {},
                             'tried': ['ln1', 'ln2', 'attn', 'merged_qkv', 'dw_qkv'],
                             'kept': ['ln1', 'ln2', 'attn', 'merged_qkv', 'dw_qkv'],
                             'skipped': {},
                             'dropped': {},
                             'minibatches': 2,
                             'attn_direct': [{'out': 0, 'dq': 0, 'dk': 0, 'dv': 0, 'attn_kb': 0}],
                             'usable': True,
                             'plan': 'ln1=True ln2=True ln_flags=0 attn=True attn_kb=0 merged_qkv=True dw_qkv=True'},
                  'warnings': [],
                  'module_runs': [(0, True), (1, True)],
                  'accum_clear': True,
                  'qdq_calls': 1},
 'opt_attention_direct_diff_missing': {'trials': ['@0',
                                                  '@1',
                                                  'attn@0',
                                                  'attn@1',
                                                  'attn,attn_kb=32@0',
                                                  'attn,attn_kb=32@1',
                                                  'attn,attn_kb=16@0',
                                                  'attn,attn_kb=16@1',
                                                  'attn@0',
                                                  'attn@1'],
                                       'plan': '',
                                       'installed': '',
                                       'report': {'errors': {},
                                                  'tried': ['attn'],
                                                  'kept': [],
                                                  'skipped': {},
                                                  'dropped': {'attn': {'0:0': -1, '0:32': -1, '0:16': -1, '1:0': -1}},
                                                  'minibatches': 2,
                                                  'attn_direct': [{'out': 0, 'dq': 0, 'dk': 0, 'attn_kb': 0},
                                                                  {'out': 0, 'dq': 0, 'dk': 0, 'attn_kb': 32},
                                                                  {'out': 0, 'dq': 0, 'dk': 0, 'attn_kb': 16},
                                                                  {'out': 0, 'dq': 0, 'dk': 0, 'attn_kb': 0}],
                                                  'usable': True,
                                                  'plan': 'ln1=False ln2=False ln_flags=0 attn=False attn_kb=0 merged_qkv=False dw_qkv=False'},
                                       'warnings': ['exact_rounding: OPTDecoderLayer: not bit-equal to the module path on this stack and left on '
                                                    "torch's own ops (slower): {'attn': {'0:0': -1, '0:32': -1, '0:16': -1, '1:0': -1}} (differing "
                                                    'values per tried pair)'],
                                       'module_runs': [(0, True), (1, True)],
                                       'accum_clear': True,
                                       'qdq_calls': 0},
 'opt_attention_key_blocks': {'trials': ['@0', '@1', 'attn@0', 'attn,attn_kb=32@0', 'attn,attn_kb=32@1', 'attn,attn_kb=16@0', 'attn,attn_kb=16@1'],
                              'plan': 'attn,attn_kb=16',
                              'installed': 'attn,attn_kb=16',
                              'report': {'errors': {},
                                         'tried': ['attn'],
                                         'kept': ['attn'],
                                         'skipped': {},
                                         'dropped': {},
                                         'minibatches': 2,
                                         'attn_direct': [{'out': 0, 'dq': 0, 'dk': 0, 'dv': 0, 'attn_kb': 0},
                                                         {'out': 0, 'dq': 0, 'dk': 0, 'dv': 2, 'attn_kb': 32},
                                                         {'out': 0, 'dq': 0, 'dk': 0, 'dv': 0, 'attn_kb': 16}],
                                         'usable': True,
                                         'plan': 'ln1=False ln2=False ln_flags=0 attn=True attn_kb=16 merged_qkv=False dw_qkv=False'},
                              'warnings': [],
                              'module_runs': [(0, True), (1, True)],
                              'accum_clear': True,
                              'qdq_calls': 0},
 'opt_attention_without_a_mask': {'trials': ['@0', '@1', 'merged_qkv@0', 'merged_qkv@1'],
                                  'plan': 'merged_qkv',
                                  'installed': 'merged_qkv',
                                  'report': {'errors': {},
                                             'tried': ['merged_qkv'],
                                             'kept': ['merged_qkv'],
                                             'skipped': {'attn': 'no additive attention mask: the call is not the one the kernel restates'},
                                             'dropped': {},
                                             'minibatches': 2,
                                             'usable': True,
                                             'plan': 'ln1=False ln2=False ln_flags=0 attn=False attn_kb=0 merged_qkv=True dw_qkv=False'},
                                  'warnings': [],
                                  'module_runs': [(0, True), (1, True)],
                                  'accum_clear': True,
                                  'qdq_calls': 0},
 'opt_base_differs_twice': {'trials': ['@0', '@0'],
                            'plan': None,
                            'installed': '',
                            'report': {'errors': {},
                                       'tried': [],
                                       'kept': [],
                                       'skipped': {},
                                       'dropped': {},
                                       'minibatches': 2,
                                       'usable': False,
                                       'base_mismatches': 3},
                            'warnings': ["exact_rounding: even with every segment on torch's own ops OPTDecoderLayer differs from the module path (3 "
                                         'values); blocks of this kind keep the module path'],
                            'module_runs': [(0, True), (1, True)],
                            'accum_clear': True,
                            'qdq_calls': 0},
 'opt_base_kept_on_second_pair': {'trials': ['@0', '@1', '@0', '@1', 'ln1@0', 'ln1@1'],
                                  'plan': 'ln1',
                                  'installed': 'ln1',
                                  'report': {'errors': {},
                                             'tried': ['ln1'],
                                             'kept': ['ln1'],
                                             'skipped': {},
                                             'dropped': {},
                                             'minibatches': 2,
                                             'kept_on_second_try': ['base'],
                                             'usable': True,
                                             'plan': 'ln1=True ln2=False ln_flags=0 attn=False attn_kb=0 merged_qkv=False dw_qkv=False'},
                                  'warnings': ['exact_rounding: OPTDecoderLayer: the all-torch form differed from the module path in its first pair '
                                               'of runs (4 values) and matched in the second pair -- the library under the comparison is not '
                                               'perfectly repeatable'],
                                  'module_runs': [(0, True), (1, True)],
                                  'accum_clear': True,
                                  'qdq_calls': 0},
 'opt_forward_all_pass': {'trials': ['', 'ln1', 'ln1', 'ln1,ln2', 'ln1,ln2', 'attn,ln1,ln2', 'attn,ln1,ln2'],
                          'plan': 'attn,ln1,ln2',
                          'installed': 'attn,ln1,ln2',
                          'report': {'usable': True,
                                     'kept': ['ln1', 'ln2', 'attn'],
                                     'plan': 'ln1=True ln2=True ln_flags=0 attn=True attn_kb=0 merged_qkv=False dw_qkv=False'},
                          'warnings': []},
 'opt_forward_base_differs_twice': {'trials': ['', ''], 'plan': None, 'installed': '', 'report': {'usable': False}, 'warnings': []},
 'opt_forward_base_passes_on_its_second_run': {'trials': ['',
                                                          '',
                                                          'ln1,ln_flags=1',
                                                          'ln1,ln_flags=1',
                                                          'ln1,ln2,ln_flags=1',
                                                          'ln1,ln2,ln_flags=1',
                                                          'attn,ln1,ln2,ln_flags=1',
                                                          'attn,ln1,ln2,ln_flags=1'],
                                               'plan': 'attn,ln1,ln2,ln_flags=1',
                                               'installed': 'attn,ln1,ln2,ln_flags=1',
                                               'report': {'usable': True,
                                                          'kept': ['ln1', 'ln2', 'attn'],
                                                          'plan': 'ln1=True ln2=True ln_flags=1 attn=True attn_kb=0 merged_qkv=False dw_qkv=False'},
                                               'warnings': []},
 'opt_forward_no_layernorm_form_and_attention_key_blocks': {'trials': ['',
                                                                       'attn',
                                                                       'attn',
                                                                       'attn,attn_kb=32',
                                                                       'attn,attn_kb=32',
                                                                       'attn,attn_kb=16',
                                                                       'attn,attn_kb=16'],
                                                            'plan': 'attn,attn_kb=16',
                                                            'installed': 'attn,attn_kb=16',
                                                            'report': {'usable': True,
                                                                       'kept': ['attn'],
                                                                       'plan': 'ln1=False ln2=False ln_flags=0 attn=True attn_kb=16 merged_qkv=False '
                                                                               'dw_qkv=False'},
                                                            'warnings': []},
 'opt_forward_second_run_differs': {'trials': ['', 'ln1', 'ln1', 'ln2', 'ln2', 'attn,ln2', 'attn,ln2'],
                                    'plan': 'attn,ln2',
                                    'installed': 'attn,ln2',
                                    'report': {'usable': True,
                                               'kept': ['ln2', 'attn'],
                                               'plan': 'ln1=False ln2=True ln_flags=0 attn=True attn_kb=0 merged_qkv=False dw_qkv=False'},
                                    'warnings': []},
 'opt_forward_without_a_mask': {'trials': ['', 'ln1', 'ln1', 'ln1,ln2', 'ln1,ln2'],
                                'plan': 'ln1,ln2',
                                'installed': 'ln1,ln2',
                                'report': {'usable': True,
                                           'kept': ['ln1', 'ln2'],
                                           'plan': 'ln1=True ln2=True ln_flags=0 attn=False attn_kb=0 merged_qkv=False dw_qkv=False'},
                                'warnings': []},
 'opt_gemm_options_get_two_attempts': {'trials': ['@0',
                                                  '@1',
                                                  'merged_qkv@0',
                                                  'merged_qkv@0',
                                                  'merged_qkv@1',
                                                  'dw_qkv,merged_qkv@0',
                                                  'dw_qkv,merged_qkv@0'],
                                       'plan': 'merged_qkv',
                                       'installed': 'merged_qkv',
                                       'report': {'errors': {},
                                                  'tried': ['merged_qkv', 'dw_qkv'],
                                                  'kept': ['merged_qkv'],
                                                  'skipped': {},
                                                  'dropped': {'dw_qkv': {'0': 8, '1': 8}},
                                                  'minibatches': 2,
                                                  'kept_on_second_try': ['merged_qkv'],
                                                  'usable': True,
                                                  'plan': 'ln1=False ln2=False ln_flags=0 attn=False attn_kb=0 merged_qkv=True dw_qkv=False'},
                                       'warnings': ['exact_rounding: OPTDecoderLayer: not bit-equal to the module path on this stack and left on '
                                                    "torch's own ops (slower): {'dw_qkv': {'0': 8, '1': 8}} (differing values per tried pair)"],
                                       'module_runs': [(0, True), (1, True)],
                                       'accum_clear': True,
                                       'qdq_calls': 0},
 'opt_kernel_option_retries_only_its_first_variant': {'trials': ['@0', '@1', 'attn@0', 'attn,attn_kb=32@0', 'attn,attn_kb=16@0', 'attn@0', 'attn@1'],
                                                      'plan': '',
                                                      'installed': '',
                                                      'report': {'errors': {},
                                                                 'tried': ['attn'],
                                                                 'kept': [],
                                                                 'skipped': {},
                                                                 'dropped': {'attn': {'0:0': 5, '0:32': 5, '0:16': 5, '1:0': 5}},
                                                                 'minibatches': 2,
                                                                 'attn_direct': [{'out': 0, 'dq': 0, 'dk': 0, 'dv': 0, 'attn_kb': 0},
                                                                                 {'out': 0, 'dq': 0, 'dk': 0, 'dv': 0, 'attn_kb': 32},
                                                                                 {'out': 0, 'dq': 0, 'dk': 0, 'dv': 0, 'attn_kb': 16},
                                                                                 {'out': 0, 'dq': 0, 'dk': 0, 'dv': 0, 'attn_kb': 0}],
                                                                 'usable': True,
                                                                 'plan': 'ln1=False ln2=False ln_flags=0 attn=False attn_kb=0 merged_qkv=False '
                                                                         'dw_qkv=False'},
                                                      'warnings': ['exact_rounding: OPTDecoderLayer: not bit-equal to the module path on this stack '
                                                                   "and left on torch's own ops (slower): {'attn': {'0:0': 5, '0:32': 5, '0:16': 5, "
                                                                   "'1:0': 5}} (differing values per tried pair)"],
                                                      'module_runs': [(0, True), (1, True)],
                                                      'accum_clear': True,
                                                      'qdq_calls': 0},
 'opt_ln_flags_first_matching': {'trials': ['@0', '@1', 'ln1,ln_flags=2@0', 'ln1,ln_flags=2@1', 'ln1,ln2,ln_flags=2@0', 'ln1,ln2,ln_flags=2@1'],
                                 'plan': 'ln1,ln2,ln_flags=2',
                                 'installed': 'ln1,ln2,ln_flags=2',
                                 'report': {'errors': {},
                                            'tried': ['ln1', 'ln2'],
                                            'kept': ['ln1', 'ln2'],
                                            'skipped': {},
                                            'dropped': {},
                                            'minibatches': 2,
                                            'usable': True,
                                            'plan': 'ln1=True ln2=True ln_flags=2 attn=False attn_kb=0 merged_qkv=False dw_qkv=False'},
                                 'warnings': [],
                                 'module_runs': [(0, True), (1, True)],
                                 'accum_clear': True,
                                 'qdq_calls': 0},
 'opt_no_layernorm_form_matches': {'trials': ['@0',
                                              '@1',
                                              'attn@0',
                                              'attn@1',
                                              'attn,merged_qkv@0',
                                              'attn,merged_qkv@1',
                                              'attn,dw_qkv,merged_qkv@0',
                                              'attn,dw_qkv,merged_qkv@1'],
                                   'plan': 'attn,dw_qkv,merged_qkv',
                                   'installed': 'attn,dw_qkv,merged_qkv',
                                   'report': {'errors': {'ln1': "no form of the LayerNorm kernel reproduces torch's row statistics / output on this "
                                                                'stack',
                                                         'ln2': "no form of the LayerNorm kernel reproduces torch's row statistics / output on this "
                                                                'stack'},
                                              'tried': ['ln1', 'ln2', 'attn', 'merged_qkv', 'dw_qkv'],
                                              'kept': ['attn', 'merged_qkv', 'dw_qkv'],
                                              'skipped': {},
                                              'dropped': {'ln1': {'stats': 'differ'}, 'ln2': {'stats': 'differ'}},
                                              'minibatches': 2,
                                              'attn_direct': [{'out': 0, 'dq': 0, 'dk': 0, 'dv': 0, 'attn_kb': 0}],
                                              'usable': True,
                                              'plan': 'ln1=False ln2=False ln_flags=0 attn=True attn_kb=0 merged_qkv=True dw_qkv=True'},
                                   'warnings': ["exact_rounding: OPTDecoderLayer: not bit-equal to the module path on this stack and left on torch's "
                                                "own ops (slower): {'ln1': {'stats': 'differ'}, 'ln2': {'stats': 'differ'}} (differing values per "
                                                'tried pair)'],
                                   'module_runs': [(0, True), (1, True)],
                                   'accum_clear': True,
                                   'qdq_calls': 0},
 'opt_one_of_two_is_dropped': {'trials': ['@0', '@1', 'ln1@0', 'ln1@1', 'ln1@0', 'ln1@1', 'ln2@0', 'ln2@1'],
                               'plan': 'ln2',
                               'installed': 'ln2',
                               'report': {'errors': {},
                                          'tried': ['ln1', 'ln2'],
                                          'kept': ['ln2'],
                                          'skipped': {},
                                          'dropped': {'ln1': {'0': 7, '1': 7}},
                                          'minibatches': 2,
                                          'usable': True,
                                          'plan': 'ln1=False ln2=True ln_flags=0 attn=False attn_kb=0 merged_qkv=False dw_qkv=False'},
                               'warnings': ["exact_rounding: OPTDecoderLayer: not bit-equal to the module path on this stack and left on torch's own "
                                            "ops (slower): {'ln1': {'0': 7, '1': 7}} (differing values per tried pair)"],
                               'module_runs': [(0, True), (1, True)],
                               'accum_clear': True,
                               'qdq_calls': 0},
 'opt_refusal': {'trials': ['@0', '@1', 'ln2@0', 'ln2@0', 'dw_qkv@0', 'dw_qkv@1'],
                 'plan': 'dw_qkv',
                 'installed': 'dw_qkv',
                 'report': {'errors': {'ln2': "RuntimeError('refused')"},
                            'tried': ['ln2', 'dw_qkv'],
                            'kept': ['dw_qkv'],
                            'skipped': {},
                            'dropped': {'ln2': {'0': -1, '1': -1}},
                            'minibatches': 2,
                            'usable': True,
                            'plan': 'ln1=False ln2=False ln_flags=0 attn=False attn_kb=0 merged_qkv=False dw_qkv=True'},
                 'warnings': ["exact_rounding: OPTDecoderLayer: not bit-equal to the module path on this stack and left on torch's own ops (slower): "
                              "{'ln2': {'0': -1, '1': -1}} (differing values per tried pair)"],
                 'module_runs': [(0, True), (1, True)],
                 'accum_clear': True,
                 'qdq_calls': 0}}
