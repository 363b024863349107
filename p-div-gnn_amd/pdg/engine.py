"""Forward/backward orchestration of EncodeProcessDecode on the HIP kernels.

One call of :meth:`EPDEngine.forward` runs the whole encode-process-decode
stack of ``gnn_local_stress/models.py:288-326`` as a fixed sequence of HIP
launches on the current stream (no host sync, no torch compute ops); with
``need_grad`` it keeps the activations the backward needs.
:meth:`EPDEngine.backward` runs the reverse sequence and accumulates every
parameter gradient into caller-provided fp32 buffers.

Per message-passing step t (weights shared across steps, models.py:313-314):

  forward                                   kernels
  x_t = LN_n(a2n_{t-1}) + x_{t-1}           pdg_node_pq      (also P = Wa x_t, Q = Wb x_t)
  e_t = LN_e(a2e_{t-1}) + e_{t-1}           pdg_edge_fwd     (C = Wc e_t + b1, both edge_net
  a1m,a2m (message), a1e,a2e (edge upd.)                      evaluations, LN partials)
  aggr = sum_dst LN_m(a2m)                  pdg_segment_sum
  a1n = relu(Wn1 [aggr, x_t] + bn1)         pdg_node_mlp1
  a2n = relu(Wn2 a1n + bn2)                 pdg_mlp2_fwd

Graph-global LayerNorm statistics are reduced by pdg_ln_finalize between the
producer and the consumer of each normalised tensor.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field

import torch

from . import hiptimer
from .lib import LN_STAT_BYTES, lib, stream_handle
from .lib import ptr as _p
from .plan import GraphPlan

L = 128
VP, IA = ctypes.c_void_p, ctypes.c_int


def _arr(ctype, values):
    """A ctypes array argument (pointer tables, row counts, leading dimensions) of a batched entry point."""
    values = list(values)
    return (ctype * len(values))(*values)


PARAM_SHAPES = [  # state_dict order of gnn_local_stress/models.py:246-286
    ("node_encoder.0.weight", (L, 6)), ("node_encoder.0.bias", (L,)),
    ("node_encoder.2.weight", (L, L)), ("node_encoder.2.bias", (L,)),
    ("node_encoder.4.weight", (L,)), ("node_encoder.4.bias", (L,)),
    ("edge_encoder.0.weight", (L, 1)), ("edge_encoder.0.bias", (L,)),
    ("edge_encoder.2.weight", (L, L)), ("edge_encoder.2.bias", (L,)),
    ("edge_encoder.4.weight", (L,)), ("edge_encoder.4.bias", (L,)),
    ("processor.edge_net.0.weight", (L, 3 * L)), ("processor.edge_net.0.bias", (L,)),
    ("processor.edge_net.2.weight", (L, L)), ("processor.edge_net.2.bias", (L,)),
    ("processor.edge_net.4.weight", (L,)), ("processor.edge_net.4.bias", (L,)),
    ("processor.node_net.0.weight", (L, 2 * L)), ("processor.node_net.0.bias", (L,)),
    ("processor.node_net.2.weight", (L, L)), ("processor.node_net.2.bias", (L,)),
    ("processor.node_net.4.weight", (L,)), ("processor.node_net.4.bias", (L,)),
    ("node_decoder.0.weight", (L, L)), ("node_decoder.0.bias", (L,)),
    ("node_decoder.2.weight", (3, L)), ("node_decoder.2.bias", (3,)),
]
PARAM_NAMES = [n for n, _ in PARAM_SHAPES]


# Kernel variants of the engine: attribute -> (A/B environment variable, shipped default).  The
# defaults are the product path, the only one the full-size parity tests (tests/test_gpu_fullsize.py)
# and the bench time; the alternatives are kept for same-box A/B timing (tools/ab_env.sh).  The rule:
# a boolean variant has a branch in the engine only while a GPU model test runs that branch against the
# default (tests/test_gpu_model.py) and tests/test_gpu_engine_launches.py pins its launch sequence; an
# A/B that is settled leaves the engine (its figures stay in EXPERIMENTS.md, its baseline kernel in the
# library, callable through the C ABI and compared by the op tests).  Tests select variants through the
# engine attributes; the environment is read only under PDG_AB=1, and a non-default value set in the
# environment without it is an error (a stray variable must not swap kernels silently).
VARIANTS = {
    # edge backward with the W2 / Wc weight gradients fused (pdg_edge_bwd_w2 / pdg_edge_gout_wc); False:
    # pdg_edge_bwd + deferred pdg_wgrad_segments passes
    "fused_edge_wgrad": ("PDG_FUSED_EDGE_WGRAD", True),
    # fused edge backward: gz1e not stored; the P/Q gather backward forms it per row as gC - gz1m (one fp32
    # rounding of |gC|) from the gC rows the Wc pass reads anyway: one E-row array written fewer per step
    "gz1e_from_gc": ("PDG_GZ1E_FROM_GC", True),
    # edge forward in the block-cooperative layout (pdg_edge_fwd_coop; 240 -> 230 us per call at config 2)
    # instead of pdg_edge_fwd
    "coop_fwd": ("PDG_EDGE_FWD_COOP", True),
    # pdg_wgrad_pairs blocks per CU (2 per CU ran as two sequential block waves at 166 VGPRs: 9.07-9.12 vs
    # 9.14-9.23 ms per config-2 step, same box)
    "pair_blocks_per_cu": ("PDG_PAIR_BLOCKS_PER_CU", 1),
    # pdg_edge_enc_fwd blocks per CU (104 VGPRs, 41 KB LDS per 8-wave block)
    "enc_blocks_per_cu": ("PDG_ENC_BLOCKS_PER_CU", 2),
}


# inference (no backward): pdg_edge_fwd_infer (16-row rounds with one barrier per round, bitwise the rows of
# pdg_edge_fwd_coop: 494 -> 446 us per 614k-edge call) from this many edges on (alone, 256 blocks: +1.5 us
# against pdg_edge_fwd_coop at 2.5k - 11k edges, equal at 27k, -3 us at 59k, -10 % from 150k edges on;
# tools/diag/efwd_sweep.py)
INFER_PIPE_MIN_EDGES = 32768


def _parse_variant(name: str, raw: str):
    env, default = VARIANTS[name]
    if isinstance(default, bool):
        if raw not in ("0", "1"):
            raise ValueError(f"{env}={raw!r}: expected 0 or 1")
        return raw == "1"
    try:
        v = int(raw)
    except ValueError:
        raise ValueError(f"{env}={raw!r}: expected an integer") from None
    if v < 1 or v > 4:
        raise ValueError(f"{env}={raw!r}: expected 1..4")
    return v


def kernel_variants(overrides: dict | None = None) -> dict:
    """The variant settings an engine starts with: the shipped defaults, the environment's A/B
    selection under PDG_AB=1 (refused without it unless every value equals the default), then
    ``overrides``."""
    out = {k: d for k, (_, d) in VARIANTS.items()}
    ab = os.environ.get("PDG_AB") == "1"
    for name, (env, default) in VARIANTS.items():
        raw = os.environ.get(env)
        if raw is None:
            continue
        val = _parse_variant(name, raw)
        if val != default and not ab:
            raise RuntimeError(f"{env}={raw} selects a non-default kernel variant of the HIP path; these are "
                               "for A/B timing only (set PDG_AB=1 to allow them), unset it to run the shipped "
                               "kernels")
        out[name] = val
    for k, v in (overrides or {}).items():
        if k not in VARIANTS:
            raise KeyError(f"unknown kernel variant {k!r} (known: {sorted(VARIANTS)})")
        out[k] = v
    return out


class _StatBuf:
    """A device array of pdg_ln_stat (or pdg_ln_bwd) structs."""

    def __init__(self, n: int, nbytes: int, device, zero: bool = True) -> None:
        # zero=False: every entry is written (pdg_ln_finalize / the producers' fused finalize) before
        # it is read, so no fill launch
        alloc = torch.zeros if zero else torch.empty
        self.buf = alloc(max(n, 1) * nbytes, dtype=torch.uint8, device=device)
        self.nbytes = nbytes

    def __getitem__(self, i: int) -> int:
        return self.buf.data_ptr() + i * self.nbytes


@dataclass
class FwdCtx:
    plan: GraphPlan
    steps: int
    scale_output: bool
    x_in: torch.Tensor = None
    e_in: torch.Tensor = None
    a1_ne: torch.Tensor = None
    a2_ne: torch.Tensor = None
    a1_ee: torch.Tensor = None
    a2_ee: torch.Tensor = None
    per_step: list = field(default_factory=list)
    x_S: torch.Tensor = None
    a1d: torch.Tensor = None
    stats: _StatBuf = None


@dataclass
class InputGrads:
    """The output buffers of the backward's opt-in input gradients (EPDEngine.backward, input_grads): fp32,
    contiguous, every element written.  ``stats8`` / ``scale_input`` as the forward took them."""
    mean_stress: torch.Tensor   # (N, 3)
    pos: torch.Tensor           # (N, 2)
    edge_attr: torch.Tensor     # (E,), in the caller's edge order
    stats8: torch.Tensor
    scale_input: bool


@dataclass
class _Fwd:
    """What one phase of the forward hands the next."""
    s: int                      # stream handle
    ctx: FwdCtx
    need_grad: bool
    # the LayerNorm whose output, plus the residual x / e, is the next step's (or the decoder's) x / e:
    # (its input a2, pointer to its statistics, its weight, its bias); the encoder's before step 0
    ln_n: tuple = None
    ln_e: tuple = None
    x: torch.Tensor = None      # x_{t-1} / e_{t-1}, the residuals (None before step 0)
    e: torch.Tensor = None
    # node LayerNorm statistics not reduced yet: pend_n block partials in pend_buf, reduced inside their
    # consumer (the next node_pq, the decoder); None: finalized already (sync mode)
    pend_n: int = None
    pend_buf: torch.Tensor = None
    Pm: torch.Tensor = None     # P = Wa x_t, Q = Wb x_t (PQm: both in the blocked layout, pdg_pq_layout)
    Qm: torch.Tensor = None
    PQm: torch.Tensor = None


@dataclass
class _Bwd:
    """What one phase of the backward hands the next."""
    s: int                      # stream handle
    G: dict                     # name -> fp32 gradient accumulator
    T: dict                     # W^T copies (EPDEngine.transposed)
    S: int                      # message-passing steps
    fused: bool                 # fused_edge_wgrad
    e_sum: bool                 # gz1e never stored: pdg_pq_scatter_bwd takes gC - gz1m
    # LayerNorm backward without finalize launches (include/pdivgnn.h, pdg_ln_colsum): every column-sum
    # producer adds its per-block rows into its group's accumulator (accs: node_net, edge_net, node encoder,
    # edge encoder) and writes per-block (S1, S2) pairs into its row of `pairs`, which the consumer reduces
    accs: tuple
    pairs: torch.Tensor
    slabs_w2: torch.Tensor = None   # weight-gradient slabs of the fused edge backward, over all steps
    slabs_wc: torch.Tensor = None
    slabs_ee: torch.Tensor = None
    # deferred weight gradients: per weight block the (G, X, rows) segments of every step
    segs: dict = field(default_factory=lambda: {k: [] for k in ("W2", "Wc", "Wa", "Wb", "Wn2", "Wn1a", "Wn1b",
                                                                 "d1", "ne2", "ee2")})
    reds: list = field(default_factory=list)         # slab reductions left to pdg_bwd_epilogue
    epi_narrow: list = field(default_factory=list)   # narrow weight-gradient finalizes for pdg_bwd_epilogue
    epi_enc: tuple = None                            # the edge encoder's first-layer sums, likewise
    # the input-gradient chain, step to step
    gx_next: torch.Tensor = None    # d loss / d x_{t+1}
    gx_t: torch.Tensor = None       # the buffer d loss / d x_t is written to (swapped with gx_next)
    ge_next: torch.Tensor = None    # d loss / d e_{t+1} (None at the last step: e_S has no consumer)
    ge_bufs: list = None
    gaggr: torch.Tensor = None
    gx_part: torch.Tensor = None
    gz1m: torch.Tensor = None
    gz1e: torch.Tensor = None
    gC_fused: torch.Tensor = None
    n_node: int = 0                 # pairs in the row of the node LayerNorm whose consumer runs next
    sync_slot: int = 0

    def PN(self, t):   # pairs of step t's node / message / edge-update LayerNorm
        return self.pairs[t]

    def PM(self, t):
        return self.pairs[self.S + t]

    def PE(self, t):
        return self.pairs[2 * self.S + t]


# the deferred weight gradients that have no pair pass: segment key, weight, its leading dimension and first
# column, bias
_DEFERRED = [
    ("W2", "processor.edge_net.2.weight", L, 0, "processor.edge_net.2.bias"),
    ("Wc", "processor.edge_net.0.weight", 3 * L, 2 * L, "processor.edge_net.0.bias"),
    ("Wn2", "processor.node_net.2.weight", L, 0, "processor.node_net.2.bias"),
    ("d1", "node_decoder.0.weight", L, 0, "node_decoder.0.bias"),
    ("ne2", "node_encoder.2.weight", L, 0, "node_encoder.2.bias"),
    ("ee2", "edge_encoder.2.weight", L, 0, "edge_encoder.2.bias"),
]


class EPDEngine:
    """Stateless executor; parameters are passed per call as a name->tensor dict."""

    def __init__(self, device: torch.device, variants: dict | None = None) -> None:
        self.device = torch.device(device)
        var = kernel_variants(variants)
        self.max_blocks = lib.pdg_max_blocks()
        self._cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        f64 = dict(dtype=torch.float64, device=self.device)
        self._part_a = torch.empty(self.max_blocks * 2, **f64)
        self._part_b = torch.empty(self.max_blocks * 2, **f64)
        self._part_col = torch.empty(self.max_blocks * 256, **f64)
        # LayerNorm backward (no finalize launches, pdg_ln_colsum in include/pdivgnn.h): per-block
        # column accumulators of the 4 LayerNorm parameter groups (node_net, edge_net, node and edge
        # encoder), rows <= the largest producer grid (2 x CUs), zeroed once per backward
        self._acc_rows = min(2 * self._cus, self.max_blocks)
        self._ln_acc = torch.zeros(4, self._acc_rows * 256, **f64)
        self._sync_pairs = torch.zeros(8, 2, **f64)
        self._part_narrow = torch.empty(self.max_blocks * (L * 6 + L + 6), **f64)
        # block partials of the two narrow gradients formed inside the encoder / decoder backward, held until
        # the backward's epilogue (apart from _part_narrow, the scratch of pdg_wgrad_narrow)
        self._part_narrow_d = torch.empty(self.max_blocks * (L * 3 + L + 3), **f64)
        self._part_narrow_ne = torch.empty(self.max_blocks * (L * 6 + L + 6), **f64)
        self._nparts = ctypes.c_int(0)
        # one weight-gradient slab per block of pdg_wgrad_segments: one 8-wave block per CU
        self._nslabs = lib.pdg_wgrad_slabs_per_cu() * self._cus
        self._nslabs_p = min(var["pair_blocks_per_cu"] * self._cus, self.max_blocks)
        # one 8-wave block per CU: the grid of the cooperative kernels and the slabs of the fused edge backward
        self._nslabs_e = min(self._cus, self.max_blocks)
        self._enc_blocks = min(var["enc_blocks_per_cu"] * self._cus, self.max_blocks)
        self._pair = torch.zeros(2, **f64)
        # slab sets of the deferred weight gradients, allocated by the first backward that needs them
        self._slab_sets: dict = {}
        self._slabs_p = None
        self.sync = None
        # the boolean kernel variants (VARIANTS above; tests and A/B tools flip these attributes)
        for k, v in var.items():
            if isinstance(v, bool):
                setattr(self, k, v)
        # the P / Q layout the library's node pre-pass writes and its cooperative edge forward reads
        self.pq_blocked = bool(lib.pdg_pq_layout())
        # optional live kernel timing: name -> list of (start, end) hiptimer.Event pairs
        self.timed: dict | None = None
        # optional backward probe (tools/grad_err_stages.py): step t -> copies of d loss / d x_t,
        # d loss / d e_t (edges in plan order) and d loss / d aggr_t
        self.probe: dict | None = None

    def variants(self) -> dict:
        """The kernel variants in effect (recorded in the bench line): every VARIANTS entry, so a new
        variant cannot be left out of the record."""
        derived = {"pair_blocks_per_cu": self._nslabs_p // self._cus,
                   "enc_blocks_per_cu": self._enc_blocks // self._cus}
        return {k: derived[k] if k in derived else getattr(self, k) for k in VARIANTS}

    def _t(self, name: str, fn, *args):
        """Launch fn(*args); when timing is enabled for `name`, bracket it with HIP events
        on the current stream (the stream every launch of this engine uses)."""
        if self.timed is None or name not in self.timed:
            return fn(*args)
        a, b = hiptimer.Event(), hiptimer.Event()   # no system-scope fence per record (pdg/hiptimer.py)
        a.record()
        r = fn(*args)
        b.record()
        self.timed[name].append((a, b))
        return r

    # ------------------------------------------------------------------ helpers
    def _empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def _finalize(self, part, count: int, out_ptr: int, s, edges: bool = False) -> None:
        if self.sync is None:
            lib.pdg_ln_finalize(part.data_ptr(), self._nparts.value, float(count), out_ptr, s)
            return
        # exact DP LayerNorm: statistics of the whole minibatch over all ranks
        group, n_glob, e_glob = self.sync
        lib.pdg_ln_partials_sum(part.data_ptr(), self._nparts.value, self._pair.data_ptr(), s)
        self._t("sync_collective", lambda: torch.distributed.all_reduce(self._pair, group=group))
        lib.pdg_ln_finalize(self._pair.data_ptr(), 1, float((e_glob if edges else n_glob) * L), out_ptr, s)

    def set_sync(self, group, n_nodes_global: int = 0, n_edges_global: int = 0) -> None:
        """Enable (group given) or disable (None) the exact data-parallel LayerNorm: every
        graph-LayerNorm of forward and backward uses the statistics of the global minibatch
        of n_nodes_global / n_edges_global rows, as one device running all of it would."""
        self.sync = None if group is None else (group, int(n_nodes_global), int(n_edges_global))

    # ------------------------------------------------------------------ forward
    def forward(self, P: dict, stats8: torch.Tensor, plan: GraphPlan, pos, mean_stress, nodes_types,
                edge_attr, steps: int, scale_input: bool, scale_output: bool, need_grad: bool):
        N, E = plan.n_nodes, plan.n_edges
        if N == 0:
            raise ValueError("empty graph")
        if steps < 1:
            raise ValueError("message_passing_steps must be >= 1")
        # E == 0 (an edgeless batch): as in the reference, every message aggregate is zero
        # (scatter of no rows), the edge branch produces empty tensors and the edge parameters get
        # zero gradients; the edge kernels are skipped
        if E == 0 and self.sync is not None:
            raise ValueError("exact (sync) data parallelism needs edges on every rank's shard")
        ctx = FwdCtx(plan=plan, steps=steps, scale_output=scale_output)
        # without edges the edge LayerNorms' entries are never finalized (zeros keep them finite)
        ctx.stats = _StatBuf(2 + 3 * steps, LN_STAT_BYTES, self.device, zero=E == 0)
        f = _Fwd(s=stream_handle(self.device), ctx=ctx, need_grad=need_grad)
        self._fwd_encode(P, f, stats8, pos, mean_stress, nodes_types, edge_attr, scale_input)
        if self.pq_blocked:   # one N x 256 array, Q's blocks 16 floats after P's (pdg_pq_layout)
            f.PQm = self._empty(N, 2 * L)
            f.Pm, f.Qm = f.PQm, f.PQm.view(-1)[16:]
        else:
            f.Pm, f.Qm = self._empty(N, L), self._empty(N, L)
        for t in range(steps):
            self._fwd_step(P, f, t)
        return self._fwd_decode(P, f, stats8), ctx

    def _fwd_encode(self, P, f: _Fwd, stats8, pos, mean_stress, nodes_types, edge_attr, scale_input) -> None:
        """Input formatting and the two encoders (models.py:308-309)."""
        ctx, s, st = f.ctx, f.s, f.ctx.stats
        N, E = ctx.plan.n_nodes, ctx.plan.n_edges
        x_in = self._empty(N, 6)
        e_in = self._empty(E)
        lib.pdg_format_inputs(N, E, _p(pos), _p(mean_stress), _p(nodes_types), _p(edge_attr), _p(ctx.plan.perm),
                              _p(stats8), int(scale_input), _p(x_in), _p(e_in), s)
        # the node encoder in the cooperative layout, one 8-wave block per CU (168 VGPRs)
        a1_ne, a2_ne = self._empty(N, L), self._empty(N, L)
        nb = self._nslabs_e
        self._t("node_enc_fwd", lib.pdg_node_enc_fwd, N, _p(x_in), _p(P["node_encoder.0.weight"]),
                _p(P["node_encoder.0.bias"]), _p(P["node_encoder.2.weight"]), _p(P["node_encoder.2.bias"]),
                _p(a1_ne), _p(a2_ne), _p(self._part_b), nb, s)
        self._nparts.value = nb
        # the node encoder's LayerNorm statistics are reduced inside step 0's node_pq (pdg_node_pq_rw_fin, as
        # every later step's; one launch fewer), its partials in _part_b until then (the edge encoder and the
        # first edge forward write _part_a / _part_b only after that node_pq)
        f.pend_buf = self._part_b
        if self.sync is None:
            f.pend_n = nb
        else:
            self._finalize(self._part_b, N * L, st[0], s)
        # the edge encoder's layer-1 output is stored only for the unfused backward (pdg_mlp2_bwd);
        # pdg_edge_enc_bwd recomputes it from the scalar input
        a1_ee = self._empty(E, L) if (f.need_grad and not self.fused_edge_wgrad) else None
        a2_ee = self._empty(E, L)
        if E and a1_ee is None:   # bf16x6 W2 product, register-stationary (pdg_edge_enc_fwd)
            nb = self._enc_blocks
            self._t("edge_enc_fwd", lib.pdg_edge_enc_fwd, E, _p(e_in), _p(P["edge_encoder.0.weight"]),
                    _p(P["edge_encoder.0.bias"]), _p(P["edge_encoder.2.weight"]), _p(P["edge_encoder.2.bias"]),
                    _p(a2_ee), _p(self._part_a), nb, s)
            self._nparts.value = nb
            self._finalize(self._part_a, E * L, st[1], s, True)
        elif E:
            lib.pdg_encoder_fwd(E, 1, _p(e_in), _p(P["edge_encoder.0.weight"]), _p(P["edge_encoder.0.bias"]),
                                _p(P["edge_encoder.2.weight"]), _p(P["edge_encoder.2.bias"]), _p(a1_ee), _p(a2_ee),
                                _p(self._part_a), ctypes.byref(self._nparts), s)
            self._finalize(self._part_a, E * L, st[1], s, True)
        if f.need_grad:
            ctx.x_in, ctx.e_in, ctx.a1_ne, ctx.a2_ne, ctx.a1_ee, ctx.a2_ee = x_in, e_in, a1_ne, a2_ne, a1_ee, a2_ee
        f.ln_n = (a2_ne, st[0], P["node_encoder.4.weight"], P["node_encoder.4.bias"])
        f.ln_e = (a2_ee, st[1], P["edge_encoder.4.weight"], P["edge_encoder.4.bias"])

    def _fwd_step(self, P, f: _Fwd, t: int) -> None:
        """Message-passing step t (models.py:313-314): node pre-pass, edge_net, aggregation, node_net."""
        ctx, s, st, need_grad = f.ctx, f.s, f.ctx.stats, f.need_grad
        plan = ctx.plan
        N, E = plan.n_nodes, plan.n_edges
        i_m, i_e, i_n = 2 + 3 * t, 3 + 3 * t, 4 + 3 * t
        ge, be = P["processor.edge_net.4.weight"], P["processor.edge_net.4.bias"]
        gn, bnn = P["processor.node_net.4.weight"], P["processor.node_net.4.bias"]
        a2n_prev, stn_prev, gn_prev, bn_prev = f.ln_n
        x_t = self._empty(N, L)
        if f.pend_n is not None:    # the previous node LayerNorm's statistics, reduced inside node_pq
            self._t("node_pq", lib.pdg_node_pq_rw_fin, N, _p(a2n_prev), f.pend_buf.data_ptr(), f.pend_n,
                    float(N * L), stn_prev, _p(gn_prev), _p(bn_prev), _p(f.x), _p(x_t),
                    _p(P["processor.edge_net.0.weight"]), _p(f.Pm), _p(f.Qm), s)
            f.pend_n = None
        else:
            self._t("node_pq", lib.pdg_node_pq_rw, N, _p(a2n_prev), stn_prev, _p(gn_prev), _p(bn_prev),
                    _p(f.x), _p(x_t), _p(P["processor.edge_net.0.weight"]), _p(f.Pm), _p(f.Qm), s)
        # the last step's edge update has no consumer (models.py:316 decodes nodes only)
        eu = t < ctx.steps - 1
        e_t = self._empty(E, L)
        a2m = self._empty(E, L)
        a1m = self._empty(E, L) if need_grad else None   # layer-1 outputs: backward only
        a2e = self._empty(E, L) if eu else None
        a1e = self._empty(E, L) if (eu and need_grad) else None
        fin_in_segsum = bool(E) and self.sync is None   # edge statistics reduced inside pdg_segment_sum_fin
        if E:
            self._fwd_edge_net(P, f, eu, e_t, a1m, a2m, a1e, a2e)
        if E and not fin_in_segsum:   # sync mode: all-reduced over the ranks
            self._finalize(self._part_a, E * L, st[i_m], s, True)
            if eu:
                self._finalize(self._part_b, E * L, st[i_e], s, True)
        # aggregation (models.py:215-217) and node_net (:240-243)
        a1n = self._empty(N, L) if need_grad else None
        a2n = self._empty(N, L)
        if E:
            aggr = self._empty(N, L)
            xs = self._empty(N, L) if need_grad else None
            if fin_in_segsum:   # + both edge LayerNorms' statistics from the edge forward's partials
                self._t("segment_sum", lib.pdg_segment_sum_fin, N, _p(plan.rowptr_dst), _p(a2m),
                        _p(self._part_a), _p(self._part_b) if eu else None, self._nparts.value, float(E * L),
                        st[i_m], st[i_e] if eu else None, _p(ge), _p(be), _p(aggr), _p(xs), s)
            else:
                self._t("segment_sum", lib.pdg_segment_sum, N, _p(plan.rowptr_dst), _p(a2m), st[i_m], _p(ge),
                        _p(be), _p(aggr), _p(xs), s)
        else:
            aggr = torch.zeros(N, L, dtype=torch.float32, device=self.device)
            xs = torch.zeros(N, L, dtype=torch.float32, device=self.device) if need_grad else None
        self._t("node_net", lib.pdg_node_net, N, _p(aggr), _p(x_t), _p(P["processor.node_net.0.weight"]),
                _p(P["processor.node_net.0.bias"]), _p(P["processor.node_net.2.weight"]),
                _p(P["processor.node_net.2.bias"]), _p(a1n), _p(a2n), _p(self._part_a),
                ctypes.byref(self._nparts), s)
        if self.sync is None:
            # finalised by the next step's node_pq, or by the decoder after the last step
            f.pend_n, f.pend_buf = self._nparts.value, self._part_a
        else:
            self._finalize(self._part_a, N * L, st[i_n], s)
        if need_grad:
            ctx.per_step.append(dict(x=x_t, e=e_t, a1m=a1m, a2m=a2m, a1e=a1e, a2e=a2e, aggr=aggr, xs=xs,
                                     a1n=a1n, a2n=a2n, i_m=i_m, i_e=i_e, i_n=i_n, eu=eu))
        f.ln_n = (a2n, st[i_n], gn, bnn)
        f.ln_e = (a2e, st[i_e], ge, be)
        f.x, f.e = x_t, e_t

    def _fwd_edge_net(self, P, f: _Fwd, eu: bool, e_t, a1m, a2m, a1e, a2e) -> None:
        """e_t and both edge_net evaluations of one step (message, and with `eu` the edge update), the
        LayerNorm partials of a2m / a2e in _part_a / _part_b (_nparts of them)."""
        plan, s = f.ctx.plan, f.s
        N, E = plan.n_nodes, plan.n_edges
        a2e_prev, ste_prev, ge_prev, be_prev = f.ln_e
        W1, b1 = P["processor.edge_net.0.weight"], P["processor.edge_net.0.bias"]
        W2, b2 = P["processor.edge_net.2.weight"], P["processor.edge_net.2.bias"]
        name = "edge_fwd" if eu else "edge_fwd_last"
        if self.coop_fwd and not f.need_grad and E >= INFER_PIPE_MIN_EDGES:
            self._t(name, lib.pdg_edge_fwd_infer, E, _p(a2e_prev), ste_prev, _p(ge_prev), _p(be_prev), _p(f.e),
                    _p(e_t), _p(plan.src), _p(plan.dst), _p(f.Pm), _p(f.Qm), _p(W1), _p(b1), _p(W2), _p(b2),
                    _p(a2m), _p(a2e), _p(self._part_a), _p(self._part_b), int(eu), self._nslabs_e, s)
            self._nparts.value = self._nslabs_e
        elif self.coop_fwd:
            self._t(name, lib.pdg_edge_fwd_coop, E, _p(a2e_prev), ste_prev, _p(ge_prev), _p(be_prev), _p(f.e),
                    _p(e_t), _p(plan.src), _p(plan.dst), _p(f.Pm), _p(f.Qm), _p(W1), _p(b1), _p(W2), _p(b2),
                    _p(a1m), _p(a2m), _p(a1e), _p(a2e), _p(self._part_a), _p(self._part_b), int(eu),
                    self._nslabs_e, s)
            self._nparts.value = self._nslabs_e
        else:
            Pu, Qu = f.Pm, f.Qm
            if self.pq_blocked:   # pdg_edge_fwd (the A/B / reference kernel) reads two N x 128 arrays
                v = f.PQm.view(N, 8, 2, 16)
                Pu, Qu = v[:, :, 0].reshape(N, L).contiguous(), v[:, :, 1].reshape(N, L).contiguous()
            self._t(name, lib.pdg_edge_fwd, E, _p(a2e_prev), ste_prev, _p(ge_prev), _p(be_prev), _p(f.e),
                    _p(e_t), _p(plan.src), _p(plan.dst), _p(Pu), _p(Qu), _p(W1), _p(b1), _p(W2), _p(b2),
                    _p(a1m), _p(a2m), _p(a1e), _p(a2e), _p(self._part_a), _p(self._part_b), int(eu),
                    ctypes.byref(self._nparts), s)

    def _fwd_decode(self, P, f: _Fwd, stats8):
        """The decoder (models.py:316-321) on x_S = LN_n(a2n_{S-1}) + x_{S-1}; with pending partials the
        last node LayerNorm's statistics are reduced inside it."""
        ctx, s = f.ctx, f.s
        N = ctx.plan.n_nodes
        a2n_prev, stn_prev, gn_prev, bn_prev = f.ln_n
        pend = f.pend_n is not None
        x_S, a1d, y = self._empty(N, L), self._empty(N, L), self._empty(N, 3)
        self._t("decoder_fwd", lib.pdg_decoder_fwd_coop, N, _p(a2n_prev), None if pend else stn_prev,
                f.pend_buf.data_ptr() if pend else None, f.pend_n or 0, float(N * L),
                stn_prev if pend else None, _p(gn_prev), _p(bn_prev), _p(f.x), _p(x_S),
                _p(P["node_decoder.0.weight"]), _p(P["node_decoder.0.bias"]), _p(a1d),
                _p(P["node_decoder.2.weight"]), _p(P["node_decoder.2.bias"]), _p(stats8), int(ctx.scale_output),
                _p(y), self._nslabs_e, s)
        if f.need_grad:
            ctx.x_S, ctx.a1d = x_S, a1d
        return y

    # ------------------------------------------------------------------ backward
    def transposed(self, P: dict) -> dict:
        """W^T copies of every weight block the backward GEMMs read."""
        s = stream_handle(self.device)
        out = {}
        jobs = []

        def tr(name, key, col0, ld):
            out[key] = T = self._empty(L, L)
            jobs.append((P[name].data_ptr() + 4 * col0, ld, T.data_ptr()))

        tr("node_decoder.0.weight", "Wd1T", 0, L)
        tr("processor.edge_net.2.weight", "W2T", 0, L)
        tr("processor.edge_net.0.weight", "WaT", 0, 3 * L)
        tr("processor.edge_net.0.weight", "WbT", L, 3 * L)
        tr("processor.edge_net.0.weight", "WcT", 2 * L, 3 * L)
        tr("processor.node_net.2.weight", "Wn2T", 0, L)
        tr("processor.node_net.0.weight", "Wn1aT", 0, 2 * L)
        tr("processor.node_net.0.weight", "Wn1bT", L, 2 * L)
        tr("node_encoder.2.weight", "Wne2T", 0, L)
        tr("edge_encoder.2.weight", "Wee2T", 0, L)
        lib.pdg_transpose128_batch(len(jobs), _arr(VP, (j[0] for j in jobs)), _arr(IA, (j[1] for j in jobs)),
                                   _arr(VP, (j[2] for j in jobs)), s)
        return out

    def backward(self, P: dict, ctx: FwdCtx, gy: torch.Tensor, G: dict,
                 input_grads: InputGrads | None = None) -> None:
        """Accumulate d(loss)/d(param) into G[name] (fp32, same shapes as P).  With ``input_grads``, also
        write d(loss)/d(mean_stress, pos, edge_attr) into its buffers (two more launches, next to the
        encoders' backward; the default launch sequence is unchanged).

        The input-gradient chain runs step by step (reverse order); the weight
        gradients of the shared 128x128 blocks are deferred: every step's row
        segments (G, X pairs, kept resident in HBM) are reduced at the end in
        one segmented MFMA pass per weight (pdg_wgrad_segments)."""
        b = self._bwd_begin(P, ctx, G)
        self._bwd_decoder(P, ctx, b, gy)
        for t in reversed(range(ctx.steps)):
            self._bwd_step(P, ctx, b, t)
        self._bwd_encoders(P, ctx, b, input_grads)
        self._bwd_wgrads(b)
        self._bwd_epilogue(b)

    # ------------------------------------------------------------------ tangent
    def tangent(self, P: dict, ctx: FwdCtx, dx_in: torch.Tensor, de_in: torch.Tensor) -> torch.Tensor:
        """The Jacobian-vector product of the forward that produced ``ctx`` (``need_grad=True``) with respect
        to its formatted inputs: ``dx_in`` (N, 6) the tangent of x_in, ``de_in`` (E,) that of e_in in plan
        order; returns d local_stress (N, 3); with ``ctx.scale_output``, ``P["_std_local_stress"]`` as in
        :meth:`backward`.  The forward linearised at the stored activations
        (csrc/pdg_tangent.hip); ``ctx`` is only read, so several tangent passes may share one forward.
        Rolling buffers only: nothing is kept per step.  The (T1, T2) pairs of every LayerNorm tangent go
        from producer to consumer in ``max_blocks`` doubles x 2, reduced inside the consumer."""
        if self.sync is not None:
            raise ValueError("the tangent pass does not run in exact (sync) data-parallel mode")
        if ctx.x_in is None:
            raise ValueError("the tangent pass needs the context of a need_grad=True forward")
        plan, S, st = ctx.plan, ctx.steps, ctx.stats
        N, E = plan.n_nodes, plan.n_edges
        if tuple(dx_in.shape) != (N, 6) or tuple(de_in.shape) != (E,):
            raise ValueError(f"dx_in must be ({N}, 6) and de_in ({E},), got {tuple(dx_in.shape)} and "
                             f"{tuple(de_in.shape)}")
        for t in (dx_in, de_in):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("dx_in / de_in must be contiguous fp32 tensors on the engine's device")
        s, nb = stream_handle(self.device), self._nslabs_e
        f64 = dict(dtype=torch.float64, device=self.device)
        # pairs: node LayerNorms, the message LayerNorm, and two for the edge LayerNorms (pdg_edge_tan reads
        # the previous step's while its blocks write this step's)
        pr_n, pr_m, pr_e0, pr_e1 = (torch.empty(2 * self.max_blocks, **f64) for _ in range(4))
        da2n, dx_a, dx_b, dP, dQ = (self._empty(N, L) for _ in range(5))
        W1e, W2e = P["processor.edge_net.0.weight"], P["processor.edge_net.2.weight"]
        g_e, g_n = P["processor.edge_net.4.weight"], P["processor.node_net.4.weight"]
        self._t("node_enc_tan", lib.pdg_node_enc_tan, N, _p(dx_in), _p(ctx.a1_ne), _p(P["node_encoder.0.weight"]),
                _p(P["node_encoder.2.weight"]), _p(ctx.a2_ne), st[0], _p(da2n), _p(pr_n), nb, s)
        if E:
            da2e_a, da2e_b, de_a, de_b, da2m = (self._empty(E, L) for _ in range(5))
            daggr = self._empty(N, L)
            self._t("edge_enc_tan", lib.pdg_edge_enc_tan, E, _p(de_in), _p(ctx.e_in), _p(P["edge_encoder.0.weight"]),
                    _p(P["edge_encoder.0.bias"]), _p(P["edge_encoder.2.weight"]), _p(ctx.a2_ee), st[1], _p(da2e_a),
                    _p(pr_e0), nb, s)
        else:   # as the forward: every message aggregate, and so its tangent, is zero
            daggr = torch.zeros(N, L, dtype=torch.float32, device=self.device)
        # the LayerNorm whose tangent, plus the residual's, is dx_t / de_t: (its input a2, its statistics, its weight)
        ln_n = (ctx.a2_ne, st[0], P["node_encoder.4.weight"])
        ln_e = (ctx.a2_ee, st[1], P["edge_encoder.4.weight"])
        dx_prev = de_prev = None
        for t in range(S):
            d = ctx.per_step[t]
            self._t("node_pre_tan", lib.pdg_node_pre_tan, N, _p(da2n), _p(ln_n[0]), ln_n[1], _p(pr_n), nb,
                    _p(ln_n[2]), _p(dx_prev), _p(dx_a), _p(W1e), _p(dP), _p(dQ), nb, s)
            if E:
                eu = d["eu"]
                self._t("edge_tan" if eu else "edge_tan_last", lib.pdg_edge_tan, E, N, _p(da2e_a), _p(ln_e[0]),
                        ln_e[1], _p(pr_e0), nb, _p(ln_e[2]), _p(de_prev), _p(de_a), _p(plan.src), _p(plan.dst),
                        _p(dP), _p(dQ), _p(W1e), _p(W2e), _p(d["a1m"]), _p(d["a2m"]), st[d["i_m"]],
                        _p(d["a1e"]) if eu else None, _p(d["a2e"]) if eu else None, st[d["i_e"]] if eu else None,
                        _p(da2m), _p(da2e_b) if eu else None, _p(pr_m), _p(pr_e1) if eu else None, int(eu), nb, s)
                self._t("segment_sum_tan", lib.pdg_segment_sum_tan, N, E, _p(plan.rowptr_dst), _p(da2m), _p(d["a2m"]),
                        st[d["i_m"]], _p(pr_m), nb, _p(g_e), _p(daggr), nb, s)
                ln_e = (d["a2e"], st[d["i_e"]], g_e)
                da2e_a, da2e_b, pr_e0, pr_e1 = da2e_b, da2e_a, pr_e1, pr_e0
                de_prev, de_a, de_b = de_a, de_b, de_a
            self._t("node_net_tan", lib.pdg_node_net_tan, N, _p(daggr), _p(dx_a), _p(P["processor.node_net.0.weight"]),
                    _p(P["processor.node_net.2.weight"]), _p(d["a1n"]), _p(d["a2n"]), st[d["i_n"]], _p(da2n), _p(pr_n),
                    nb, s)
            ln_n = (d["a2n"], st[d["i_n"]], g_n)
            dx_prev, dx_a, dx_b = dx_a, dx_b, dx_a
        dy = self._empty(N, 3)
        self._t("decoder_tan", lib.pdg_decoder_tan, N, _p(da2n), _p(ln_n[0]), ln_n[1], _p(pr_n), nb, _p(ln_n[2]),
                _p(dx_prev), _p(P["node_decoder.0.weight"]), _p(ctx.a1d), _p(P["node_decoder.2.weight"]),
                _p(P["_std_local_stress"]) if ctx.scale_output else None, int(ctx.scale_output), _p(dy), nb, s)
        return dy

    def _bwd_begin(self, P, ctx: FwdCtx, G) -> _Bwd:
        """W^T copies, the fused edge backward's slabs, the LayerNorm accumulators and pair rows."""
        E, S = ctx.plan.n_edges, ctx.steps
        T = self.transposed(P)
        fused = self.fused_edge_wgrad
        b = _Bwd(s=stream_handle(self.device), G=G, T=T, S=S, fused=fused, e_sum=fused and self.gz1e_from_gc,
                 accs=None, pairs=None)
        if fused:
            # the three fused weight-gradient slab sets (W2, Wc, the edge encoder's W2) are written by the
            # first call of the backward (slab_init) and need no fill; the LayerNorm column-sum
            # accumulators are zeroed (one fill launch)
            # (an edgeless batch runs no edge kernel: zeros, so the edge weights get zero gradients)
            sl = (torch.empty if E else torch.zeros)(3, self._nslabs_e, L * L + L, dtype=torch.float32,
                                                     device=self.device)
            b.slabs_w2, b.slabs_wc, b.slabs_ee = sl[0], sl[1], sl[2]
            acc = torch.zeros(self._ln_acc.shape, dtype=torch.float64, device=self.device)
        else:
            acc = self._ln_acc
            acc.zero_()
        b.accs = tuple(acc[i] for i in range(4))
        b.pairs = torch.empty(3 * S + 2, self.max_blocks * 2, dtype=torch.float64, device=self.device)
        return b

    def _pairs_src(self, b: _Bwd, pp, n: int):
        """(pairs pointer, count) for a consumer; sync DP mode reduces them first and
        all-reduces the (S1, S2) pair over the ranks (global-minibatch LayerNorm)."""
        if self.sync is None:
            return _p(pp), n
        out = self._sync_pairs[b.sync_slot % 8]
        b.sync_slot += 1
        lib.pdg_ln_partials_sum(_p(pp), n, _p(out), b.s)
        self._t("sync_collective", lambda: torch.distributed.all_reduce(out, group=self.sync[0]))
        return _p(out), 1

    def _ln_producing(self, P, ctx: FwdCtx, b: _Bwd, kind: str, t: int):
        """The LayerNorm whose output, plus the residual, is x_t (kind "n") or e_t (kind "e"): step t-1's
        node_net / edge_net LayerNorm, or at t == 0 the encoder's.  Returns (its column-sum accumulator,
        its row of pairs, its input a2, pointer to its statistics, its weight)."""
        st = ctx.stats
        if t > 0:
            d = ctx.per_step[t - 1]
            if kind == "n":
                return b.accs[0], b.PN(t - 1), d["a2n"], st[d["i_n"]], P["processor.node_net.4.weight"]
            return b.accs[1], b.PE(t - 1), d["a2e"], st[d["i_e"]], P["processor.edge_net.4.weight"]
        if kind == "n":
            return b.accs[2], b.pairs[3 * b.S], ctx.a2_ne, st[0], P["node_encoder.4.weight"]
        return b.accs[3], b.pairs[3 * b.S + 1], ctx.a2_ee, st[1], P["edge_encoder.4.weight"]

    def _edge_ln_pairs(self, ctx: FwdCtx, b: _Bwd, pp, gy_rows, a2, st_ptr, acc, g):
        """(pairs pointer, count), for its consumer, of a LayerNorm that produced an edge state e with
        gy_rows = d loss / d e: the fused backward has the pairs from the pdg_edge_gout_wc that wrote
        gy_rows (one block per CU), the unfused one runs pdg_ln_colsum."""
        if b.fused:
            return self._pairs_src(b, pp, self._nslabs_e)
        lib.pdg_ln_colsum(ctx.plan.n_edges, _p(gy_rows), None, _p(a2), st_ptr, _p(acc),
                          ctypes.byref(self._nparts), _p(g), _p(pp), 1, b.s)
        return self._pairs_src(b, pp, self._nparts.value)

    def _bwd_decoder(self, P, ctx: FwdCtx, b: _Bwd, gy) -> None:
        """The decoder's backward, and the buffers of the input-gradient chain."""
        N, E, S, nse = ctx.plan.n_nodes, ctx.plan.n_edges, b.S, self._nslabs_e
        gy = gy.contiguous()
        if ctx.scale_output:
            gy = gy * P["_std_local_stress"]
        gz1d, gx = self._empty(N, L), self._empty(N, L)
        dl = ctx.per_step[S - 1]
        # + the column sums of the last node LayerNorm (upstream gradient: gx; for the earlier steps the next
        # step's pdg_gemm_sum2_coop produces them), + node_decoder.2's weight / bias gradient from the same
        # a1d / gy rows (block partials)
        self._t("decoder_bwd", lib.pdg_decoder_bwd_coop, N, _p(gy), _p(ctx.a1d), _p(P["node_decoder.2.weight"]),
                _p(b.T["Wd1T"]), _p(gz1d), _p(gx), _p(dl["a2n"]), ctx.stats[dl["i_n"]], _p(b.accs[0]),
                _p(P["processor.node_net.4.weight"]), _p(b.PN(S - 1)), 1, _p(self._part_narrow_d), nse, b.s)
        b.epi_narrow.append((self._part_narrow_d, nse, 3, 1, b.G["node_decoder.2.weight"], None,
                             b.G["node_decoder.2.bias"]))
        b.segs["d1"].append((gz1d, ctx.x_S, N))
        b.gaggr, b.gx_part, b.gx_t = (self._empty(N, L) for _ in range(3))
        b.gz1m = self._empty(E, L)
        b.gz1e = None if b.e_sum else self._empty(E, L)
        b.ge_bufs = [self._empty(E, L), self._empty(E, L)]
        b.gC_fused = self._empty(E, L) if b.fused else None
        b.gx_next, b.n_node = gx, nse

    def _bwd_step(self, P, ctx: FwdCtx, b: _Bwd, t: int) -> None:
        """Step t's input gradients: node_net backward, edge backward + P/Q gather backward, then
        gx_t (pdg_gemm_sum2_coop); its weight-gradient segments are queued."""
        N, E, T, s, nse = ctx.plan.n_nodes, ctx.plan.n_edges, b.T, b.s, self._nslabs_e
        d = ctx.per_step[t]
        eu, fused = d["eu"], b.fused
        assert E == 0 or eu == (b.ge_next is not None)
        gz2n, gz1n, gP, gQ = (self._empty(N, L) for _ in range(4))
        gC = b.gC_fused if fused else self._empty(E, L)   # fused: consumed within the step
        if fused and not eu:
            gC = b.gz1m   # message branch only: gC = gz1m, written once (pdg_edge_bwd_w2)
        gz2m = None if fused else self._empty(E, L)
        gz2e = self._empty(E, L) if (eu and not fused) else None
        ge_out = b.ge_bufs[t % 2]
        # node_net backward (n_t = LN_n(a2n_t), gy = gx_next; x_{t+1} = n_t + x_t), three W^T products in bf16x6
        pn, nn = self._pairs_src(b, b.PN(t), b.n_node)
        self._t("node_bwd", lib.pdg_node_bwd_coop, N, _p(b.gx_next), _p(d["a2n"]), _p(d["a1n"]),
                ctx.stats[d["i_n"]], None, _p(P["processor.node_net.4.weight"]), _p(T["Wn2T"]), _p(T["Wn1aT"]),
                _p(T["Wn1bT"]), _p(gz2n), _p(gz1n), _p(b.gaggr), _p(b.gx_part), pn, nn, nse, s)
        if E == 0:             # no edge: P and Q feed nothing (models.py:215-222 on empty tensors)
            gP.zero_()
            gQ.zero_()
        else:
            self._bwd_edge_net(P, ctx, b, t, gC, gz2m, gz2e, ge_out, gP, gQ)
        # gx_t in bf16x6, with the column sums / pairs of the LayerNorm whose output it is the gradient of
        acc, pp, a2n_prev, st_prev, gl = self._ln_producing(P, ctx, b, "n", t)
        self._t("gemm_sum2", lib.pdg_gemm_sum2_coop, N, _p(gP), _p(gQ), _p(T["WaT"]), _p(T["WbT"]),
                _p(b.gx_part), _p(b.gx_t), _p(a2n_prev), st_prev, _p(acc), _p(gl), _p(pp), 1, nse, s)
        b.n_node = nse
        segs = b.segs
        if not fused and E:
            segs["W2"].append((gz2m, d["a1m"], E))
            if eu:
                segs["W2"].append((gz2e, d["a1e"], E))
            segs["Wc"].append((gC, d["e"], E))
        segs["Wa"].append((gP, d["x"], N))
        segs["Wb"].append((gQ, d["x"], N))
        segs["Wn2"].append((gz2n, d["a1n"], N))
        segs["Wn1a"].append((gz1n, d["aggr"], N))
        segs["Wn1b"].append((gz1n, d["x"], N))
        if self.probe is not None:
            self.probe[t] = dict(gx=b.gx_t.clone(), ge=ge_out.clone() if E else None, gaggr=b.gaggr.clone())
        b.gx_next, b.gx_t = b.gx_t, b.gx_next
        b.ge_next = ge_out

    def _bwd_edge_net(self, P, ctx: FwdCtx, b: _Bwd, t: int, gC, gz2m, gz2e, ge_out, gP, gQ) -> None:
        """Both edge_net evaluations of step t backwards (E > 0): ge_out = d loss / d e_t, and gP / gQ
        through the P/Q gather; fused, also the W2 / Wc weight gradients (slabs)."""
        plan, T, s, nse = ctx.plan, b.T, b.s, self._nslabs_e
        N, E, st = plan.n_nodes, plan.n_edges, ctx.stats
        d = ctx.per_step[t]
        eu, last = d["eu"], int(t == b.S - 1)
        g_edge = P["processor.edge_net.4.weight"]
        # message LayerNorm: gy = gaggr[dst], summed per node with the forward's sum of xhat
        lib.pdg_ln_colsum_nodes(N, _p(b.gaggr), _p(plan.rowptr_dst), _p(d["xs"]), _p(b.accs[1]),
                                ctypes.byref(self._nparts), _p(g_edge), _p(b.PM(t)), 1, s)
        pm, nm = self._pairs_src(b, b.PM(t), self._nparts.value)
        pe, ne = None, 0
        if eu:   # edge-update LayerNorm: gy = ge_next (per edge)
            pe, ne = self._edge_ln_pairs(ctx, b, b.PE(t), b.ge_next, d["a2e"], st[d["i_e"]], b.accs[1], g_edge)
        if b.fused:
            self._t("edge_bwd" if eu else "edge_bwd_last", lib.pdg_edge_bwd_w2, E, _p(plan.dst), _p(b.gaggr),
                    _p(b.ge_next), _p(d["a2m"]), _p(d["a1m"]), _p(d["a2e"]), _p(d["a1e"]), st[d["i_m"]],
                    st[d["i_e"]] if eu else None, None, None, _p(g_edge), _p(T["W2T"]), _p(b.gz1m),
                    _p(b.gz1e if eu else None), _p(gC), _p(b.slabs_w2), nse, pm, nm, pe, ne, last, s)
            # the edge-update rows of the P/Q gather backward: gz1e, or gC (= gz1m + gz1e) with e_is_sum
            ge_rows, e_is_sum = (gC, 1) if (b.e_sum and eu) else (b.gz1e if eu else None, 0)
        else:
            self._t("edge_bwd" if eu else "edge_bwd_last", lib.pdg_edge_bwd, E, _p(plan.dst), _p(b.gaggr),
                    _p(b.ge_next), _p(d["a2m"]), _p(d["a1m"]), _p(d["a2e"]), _p(d["a1e"]), st[d["i_m"]],
                    st[d["i_e"]] if eu else None, None, None, _p(g_edge), _p(T["W2T"]), _p(T["WcT"]),
                    _p(gz2m), _p(b.gz1m), _p(gz2e), _p(b.gz1e if eu else None), _p(gC), _p(ge_out), pm, nm, pe,
                    ne, s)
            ge_rows, e_is_sum = b.gz1e if eu else None, 0
        # the P/Q gather backward before the Wc pass: gz1m / gz1e are re-read while still in the Infinity Cache
        self._t("pq_scatter_bwd", lib.pdg_pq_scatter_bwd, N, _p(plan.rowptr_dst), _p(plan.rowptr_src),
                _p(plan.perm_src), _p(b.gz1m), _p(ge_rows), e_is_sum, _p(gP), _p(gQ), s)
        if b.fused:
            # ge_out and the Wc weight gradient, + the column sums / pairs of the LayerNorm that produced e_t
            acc, pp, a2ln, st_ln, gl = self._ln_producing(P, ctx, b, "e", t)
            self._t("edge_gout", lib.pdg_edge_gout_wc, E, _p(gC), _p(d["e"]), _p(b.ge_next), _p(T["WcT"]),
                    _p(ge_out), _p(b.slabs_wc), nse, _p(a2ln), st_ln, _p(acc), _p(gl), _p(pp), 1, last, s)

    def _bwd_encoders(self, P, ctx: FwdCtx, b: _Bwd, ig: InputGrads | None = None) -> None:
        """The two encoders' backward; their narrow first-layer gradients go to the epilogue (fused) or
        pdg_wgrad_narrow.  With `ig`, the input gradients from the same operands (pdg_node_enc_gin /
        pdg_edge_enc_gin, each issued before the call whose operands it shares)."""
        N, E, T, G, s, nse = ctx.plan.n_nodes, ctx.plan.n_edges, b.T, b.G, b.s, self._nslabs_e
        gz2 = self._empty(N, L)
        _, pp, a2, st_ln, gl = self._ln_producing(P, ctx, b, "n", 0)
        pn, nn = self._pairs_src(b, pp, b.n_node)
        if ig is not None:
            self._t("node_enc_gin", lib.pdg_node_enc_gin, N, _p(b.gx_next), _p(a2), _p(ctx.a1_ne),
                    _p(P["node_encoder.0.weight"]), st_ln, None, pn, nn, _p(gl), _p(T["Wne2T"]), _p(ig.stats8),
                    int(ig.scale_input), _p(ig.mean_stress), _p(ig.pos), nse, s)
        # bf16x6 (pdg_mlp2_bwd_coop), + the first layer's weight / bias gradient from gz1 and the encoder
        # input (block partials; gz1 is not stored)
        self._t("node_enc_bwd", lib.pdg_mlp2_bwd_coop, N, _p(b.gx_next), _p(a2), _p(ctx.a1_ne), st_ln, None,
                _p(gl), _p(T["Wne2T"]), _p(gz2), None, pn, nn, _p(ctx.x_in), _p(self._part_narrow_ne), nse, s)
        b.epi_narrow.append((self._part_narrow_ne, nse, 6, 0, G["node_encoder.0.weight"],
                             G["node_encoder.0.bias"], None))
        b.segs["ne2"].append((gz2, ctx.a1_ne, N))
        if not E:
            return
        acc, pp, a2, st_ln, gl = self._ln_producing(P, ctx, b, "e", 0)
        pe, ne = self._edge_ln_pairs(ctx, b, pp, b.ge_next, a2, st_ln, acc, gl)
        if ig is not None:   # the layer-1 output recomputed from e_in, whichever backward variant runs
            self._t("edge_enc_gin", lib.pdg_edge_enc_gin, E, _p(b.ge_next), _p(a2), _p(ctx.e_in),
                    _p(P["edge_encoder.0.weight"]), _p(P["edge_encoder.0.bias"]), st_ln, None, pe, ne, _p(gl),
                    _p(T["Wee2T"]), _p(ctx.plan.perm), _p(ig.stats8), int(ig.scale_input), _p(ig.edge_attr), nse, s)
        if b.fused:   # one pass: weight gradients in slabs, the 1 -> 128 layer's as per-block sums
            nsum = torch.empty(nse, 2 * L, dtype=torch.float64, device=self.device)
            self._t("edge_enc_bwd", lib.pdg_edge_enc_bwd, E, _p(b.ge_next), _p(a2), _p(ctx.e_in),
                    _p(P["edge_encoder.0.weight"]), _p(P["edge_encoder.0.bias"]), st_ln, None, pe, ne,
                    _p(gl), _p(T["Wee2T"]), _p(b.slabs_ee), _p(nsum), nse, 1, s)
            b.reds.append((b.slabs_ee, nse, G["edge_encoder.2.weight"], L, 0, G["edge_encoder.2.bias"]))
            b.epi_enc = (nsum, nse, G["edge_encoder.0.weight"], G["edge_encoder.0.bias"])
        else:
            gz2e, gz1e = self._empty(E, L), self._empty(E, L)
            lib.pdg_mlp2_bwd(E, _p(b.ge_next), None, _p(a2), _p(ctx.a1_ee), st_ln, None, _p(gl), _p(T["Wee2T"]),
                             _p(gz2e), _p(gz1e), pe, ne, s)
            b.segs["ee2"].append((gz2e, ctx.a1_ee, E))
            lib.pdg_wgrad_narrow(E, _p(gz1e), _p(ctx.e_in), 1, 0, _p(self._part_narrow),
                                 _p(G["edge_encoder.0.weight"]), _p(G["edge_encoder.0.bias"]), None, s)

    def _reduce(self, b: _Bwd, slabs, n: int, wname: str, ld: int, col0: int, bname, later: bool) -> None:
        """Add a slab set into G[wname][:, col0:col0+128] (and G[bname]): in the epilogue, or at once where
        the next chunk overwrites the slabs."""
        job = (slabs, n, b.G[wname], ld, col0, b.G[bname] if bname else None)
        if later:
            b.reds.append(job)
        else:
            lib.pdg_wgrad_reduce(_p(slabs), n, _p(job[2]), ld, col0, _p(job[5]), b.s)

    def _bwd_wgrads(self, b: _Bwd) -> None:
        """The deferred weight gradients: one segmented pass + slab reduction per shared weight block."""
        self._wgrad_pairs(b)
        self._wgrad_segments(b)
        if b.fused:   # the slabs of the fused edge backward, accumulated over all steps
            self._reduce(b, b.slabs_w2, self._nslabs_e, "processor.edge_net.2.weight", L, 0,
                         "processor.edge_net.2.bias", True)
            self._reduce(b, b.slabs_wc, self._nslabs_e, "processor.edge_net.0.weight", 3 * L, 2 * L,
                         "processor.edge_net.0.bias", True)

    def _wgrad_pairs(self, b: _Bwd) -> None:
        """The weight pairs that share an operand, one pass each (pdg_wgrad_pairs): Wa / Wb against x
        (gP, gQ), node_net.0's halves from gz1n (against aggr, x); at most 32 segments per launch."""
        segs, nsp = b.segs, self._nslabs_p
        if self._slabs_p is None:
            self._slabs_p = torch.empty(2, 2, nsp, L * L + L, dtype=torch.float32, device=self.device)
        pair_sets = [
            (1, [(g, q, x, n) for (g, x, n), (q, _, _) in zip(segs["Wa"], segs["Wb"])],
             ("processor.edge_net.0.weight", 3 * L, 0, None), ("processor.edge_net.0.weight", 3 * L, L, None)),
            (0, [(g, a, x, n) for (g, a, n), (_, x, _) in zip(segs["Wn1a"], segs["Wn1b"])],
             ("processor.node_net.0.weight", 2 * L, 0, "processor.node_net.0.bias"),
             ("processor.node_net.0.weight", 2 * L, L, None)),
        ]
        for gi, (shx, sl, w0, w1) in enumerate(pair_sets):
            sp0, sp1 = self._slabs_p[gi]
            later = len(sl) <= 32   # one chunk: nothing overwrites the slabs before the epilogue
            for c0 in range(0, len(sl), 32):
                chunk = sl[c0:c0 + 32]
                self._t("wgrad_pair", lib.pdg_wgrad_pairs, len(chunk), _arr(VP, (c[0].data_ptr() for c in chunk)),
                        _arr(VP, (c[1].data_ptr() for c in chunk)), _arr(VP, (c[2].data_ptr() for c in chunk)),
                        _arr(IA, (c[3] for c in chunk)), shx, _p(sp0), _p(sp1), nsp, b.s)
                self._reduce(b, sp0, nsp, *w0, later)
                self._reduce(b, sp1, nsp, *w1, later)

    def _slab_set(self, key: str):
        """The slab set of one deferred weight, allocated the first time that weight has a segment pass:
        with the fused edge backward and the pair passes only node_net.2, the decoder and the node encoder
        need one."""
        if key not in self._slab_sets:
            self._slab_sets[key] = torch.empty(self._nslabs, L * L + L, dtype=torch.float32, device=self.device)
        return self._slab_sets[key]

    def _wgrad_segments(self, b: _Bwd) -> None:
        """The other deferred weights (pdg_wgrad_segments): those of at most 32 segments up to three per
        launch, their reductions left to the epilogue; the larger ones in chunks of 32 segments, each
        reduced at once (the next chunk overwrites the slab set)."""
        segs, ns, s = b.segs, self._nslabs, b.s
        small = [r for r in _DEFERRED if 0 < len(segs[r[0]]) <= 32]
        for c0 in range(0, len(small), 3):
            grp = small[c0:c0 + 3]
            flat = [seg for r in grp for seg in segs[r[0]]]
            self._t("wgrad_batch", lib.pdg_wgrad_segments_batch, len(grp),
                    _arr(IA, (len(segs[r[0]]) for r in grp)), _arr(VP, (g.data_ptr() for g, _, _ in flat)),
                    _arr(VP, (x.data_ptr() for _, x, _ in flat)), _arr(IA, (n for _, _, n in flat)),
                    _arr(VP, (_p(self._slab_set(r[0])) for r in grp)), ns, s)
            for key, wname, ld, col0, bname in grp:
                self._reduce(b, self._slab_set(key), ns, wname, ld, col0, bname, True)
        for key, wname, ld, col0, bname in _DEFERRED:
            sl = segs[key]
            if len(sl) <= 32:
                continue
            slabs = self._slab_set(key)
            for c0 in range(0, len(sl), 32):
                chunk = sl[c0:c0 + 32]
                self._t("wgrad_" + key, lib.pdg_wgrad_segments, len(chunk),
                        _arr(VP, (g.data_ptr() for g, _, _ in chunk)), _arr(VP, (x.data_ptr() for _, x, _ in chunk)),
                        _arr(IA, (n for _, _, n in chunk)), _p(slabs), ns, s)
                self._reduce(b, slabs, ns, wname, ld, col0, bname, False)

    def _bwd_epilogue(self, b: _Bwd) -> None:
        """Every end-of-backward reduction in one launch (pdg_bwd_epilogue): the deferred slab reductions,
        the LayerNorm weight / bias gradients of the four accumulator groups, the narrow weight gradients
        and the edge encoder's first layer (more than 16 slab sets: the rest in pdg_wgrad_reduce_batch)."""
        G, reds, narrow, enc = b.G, b.reds, b.epi_narrow, b.epi_enc
        for c0 in range(16, len(reds), 16):
            jb = reds[c0:c0 + 16]
            lib.pdg_wgrad_reduce_batch(len(jb), _arr(VP, (_p(j[0]) for j in jb)), _arr(IA, (j[1] for j in jb)),
                                       _arr(VP, (_p(j[2]) for j in jb)), _arr(IA, (j[3] for j in jb)),
                                       _arr(IA, (j[4] for j in jb)), _arr(VP, (_p(j[5]) for j in jb)), b.s)
        jb = reds[:16]
        names = ("processor.node_net.4", "processor.edge_net.4", "node_encoder.4", "edge_encoder.4")
        lib.pdg_bwd_epilogue(len(jb), _arr(VP, (_p(j[0]) for j in jb)), _arr(IA, (j[1] for j in jb)),
                             _arr(VP, (_p(j[2]) for j in jb)), _arr(IA, (j[3] for j in jb)),
                             _arr(IA, (j[4] for j in jb)), _arr(VP, (_p(j[5]) for j in jb)),
                             4, _arr(VP, (_p(a) for a in b.accs)), _arr(IA, [self._acc_rows] * 4),
                             _arr(VP, (_p(G[k + ".weight"]) for k in names)),
                             _arr(VP, (_p(G[k + ".bias"]) for k in names)),
                             len(narrow), _arr(VP, (_p(j[0]) for j in narrow)), _arr(IA, (j[1] for j in narrow)),
                             _arr(IA, (j[2] for j in narrow)), _arr(IA, (j[3] for j in narrow)),
                             _arr(VP, (_p(j[4]) for j in narrow)), _arr(VP, (_p(j[5]) for j in narrow)),
                             _arr(VP, (_p(j[6]) for j in narrow)),
                             _p(enc[0]) if enc else None, enc[1] if enc else 0,
                             _p(enc[2]) if enc else None, _p(enc[3]) if enc else None, b.s)
