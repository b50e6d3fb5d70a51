"""Shared helpers of the stream tests (tests/test_branch_streams_gpu.py, tests/test_stream_contract_gpu.py): a calibrated
device-side delay, exact (bit-pattern) comparison, a snapshot of everything a forward + backward leaves behind, and the
model / batch the side-stream tests run.  No test functions here.

The only delay used anywhere in these tests is torch.cuda._sleep on the stream to be held back: a spin kernel of torch's
own that touches no memory.  Its length is a CONDITION (long enough that everything the other streams can run without the
delayed one has finished), derived from durations the tests measure themselves — never a tuned number."""
import sys
import warnings

import torch

DEV = torch.device("cuda", 0)
BATCH = 8                      # the smallest batch the graph tests use: ragged lengths, compact drug-token block, ProteinCNN plan,
BATCH_SEED = 7                 # train-mode BatchNorm

_cycles_per_ms = None


def calibrate_sleep() -> float:
    """Cycles of torch.cuda._sleep per millisecond on this device: one timed sleep between an event pair, cached."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        cycles = 2_000_000
        torch.cuda._sleep(1000)                  # (the spin kernel's first launch loads its code object)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, "torch.cuda._sleep(%d) took %.4f ms: too short to calibrate a delay with" % (cycles, ms)
        _cycles_per_ms = cycles / ms
    return _cycles_per_ms


def skew(stream, ms: float) -> None:
    """Hold `stream` back by about `ms` milliseconds: everything enqueued on it afterwards starts that much later."""
    cycles = int(ms * calibrate_sleep())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def runs_beside(held, other, ms: float = 2.0) -> bool:
    """True when work enqueued on `other` finishes while `held` is asleep.  Two streams need not be concurrent: the runtime
    maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES), and two streams of one queue run in turn — a delay on one
    then delays the other and the skew shows nothing."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(other):
        e0.record()
    skew(held, ms)
    with torch.cuda.stream(other):
        torch.cuda._sleep(10)
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) < 0.5 * ms


def side_streams(n: int = 1, tries: int = 24) -> tuple:
    """n fresh streams, each of which runs beside the current stream and beside the others (probed with runs_beside, both
    ways) — what a skewed run needs for its delay to mean anything.  Where the device does not give that many (fewer hardware queues
    than streams) the rest are plain fresh streams and a warning says so: the comparison stays valid, the skew shows less."""
    chosen, cur = [], torch.cuda.current_stream()
    for _ in range(tries):
        s = torch.cuda.Stream()
        if all(runs_beside(t, s) and runs_beside(s, t) for t in [cur] + chosen):
            chosen.append(s)
            if len(chosen) == n:
                return tuple(chosen)
    warnings.warn("only %d of %d streams run beside the current stream and each other (GPU_MAX_HW_QUEUES too small?)" % (len(chosen), n))
    return tuple(chosen + [torch.cuda.Stream() for _ in range(n - len(chosen))])


def measure_ms(fn) -> float:
    """Device time of fn() on the current stream, once, between an event pair (fn has run before: nothing is compiled or
    allocated for the first time inside the measurement)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def delay_for(plain_ms: float) -> float:
    """The delay of a skewed run: twice the measured plain duration of what runs beside it, at least 5 ms."""
    return max(2.0 * plain_ms, 5.0)


_INT_VIEW = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t: torch.Tensor) -> torch.Tensor:
    """The integer view of a tensor's bit patterns (bf16 -> int16, fp32 -> int32, ...): exact comparison, NaN included."""
    t = t.detach()
    if t.is_floating_point():
        return t.contiguous().view(_INT_VIEW[t.element_size()])
    return t


def _flatten(prefix, v, out):
    if torch.is_tensor(v):
        out[prefix] = bits(v).clone()
    elif isinstance(v, dict):
        for k in v:
            _flatten("%s.%s" % (prefix, k), v[k], out)
    elif isinstance(v, (tuple, list)):
        out[prefix + ".len"] = len(v)
        for i, x in enumerate(v):
            _flatten("%s.%d" % (prefix, i), x, out)
    else:
        out[prefix] = v                        # None, an int (a block size), a str (a mode)


def snapshot_outputs(model, outs) -> dict:
    """Cloned bits of every tensor in the forward's returned tuple (nested dicts / pairs flattened) and of the kept attention
    maps.  The clones are enqueued on the CURRENT stream and nothing synchronises first: a result the forward handed back
    without joining its stream is read early, as a caller would read it."""
    snap = {}
    _flatten("out", tuple(outs), snap)
    for name in ("A_v_gca", "A_x_gca", "P_v_gca", "P_x_gca"):
        _flatten(name, getattr(model, name, None), snap)
    return snap


def snapshot_state(model) -> dict:
    """Cloned bits of every parameter's .grad and of every buffer (the BatchNorm running_mean / running_var /
    num_batches_tracked among them)."""
    snap = {}
    for name, p in model.named_parameters():
        _flatten("grad." + name, p.grad, snap)
    for name, b in model.named_buffers():
        _flatten("buf." + name, b, snap)
    return snap


def snapshot(model, outs) -> dict:
    """name -> cloned bits of all a forward (+ backward) leaves: snapshot_outputs and snapshot_state."""
    snap = snapshot_outputs(model, outs)
    snap.update(snapshot_state(model))
    torch.cuda.synchronize()
    return snap


def differing_keys(a: dict, b: dict) -> list:
    """[(key, what differs)] — empty when the two snapshots are equal bit for bit, key by key."""
    bad = [(k, "only in one snapshot") for k in sorted(set(a) ^ set(b))]
    for k in a:
        if k not in b:
            continue
        x, y = a[k], b[k]
        if torch.is_tensor(x) and torch.is_tensor(y):
            if x.shape != y.shape or x.dtype != y.dtype:
                bad.append((k, "%s %s vs %s %s" % (tuple(x.shape), x.dtype, tuple(y.shape), y.dtype)))
            elif not torch.equal(x, y):
                bad.append((k, "%d of %d elements differ" % (int((x != y).sum()), x.numel())))
        elif torch.is_tensor(x) or torch.is_tensor(y) or x != y:
            bad.append((k, "%r vs %r" % (type(x).__name__, type(y).__name__)))
    return bad


def assert_same(a: dict, b: dict, what: str = "") -> None:
    bad = differing_keys(a, b)
    assert not bad, "%s: %d of %d keys differ: %s" % (what, len(bad), len(a), bad[:12])


# ---- the model and the batch ------------------------------------------------------------------------------------------------
def make_model(kind: str, dtype, dropout: bool = False, state=None, graph_steps=False):
    """(model, cfg, trainer): the deterministic fixture weights of tests/test_model_gpu.py's build() (the MolecularGCN keeps its
    own, seeded, initialisation), on the device, inside a Trainer (world 1; eager unless graph_steps) — the owner of hints_of.  dropout=False
    zeroes every dropout probability as build() does; True leaves the configs' own.  state: a state_dict to load instead."""
    from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
    from druglamp_amd.model import MInterface
    from druglamp_amd.trainer import Trainer
    from tests.helpers import det_state_dict, load
    torch.manual_seed(1234)
    cfg = load_yaml_into(get_cfg_defaults(), kind)
    m = MInterface(kind, cfg).load_model(n_drug_feature=384, n_prot_feature=640)
    if state is None:
        state = det_state_dict(load("model_" + kind))
        own = m.state_dict()
        for k in own:
            if k.startswith("drug_extractor."):
                state[k] = own[k]
    m.load_state_dict(state, strict=True)
    if not dropout:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        m.pmma.p_drop = 0.0
        m.pmma.embeddings.p_drop = 0.0
    m = m.to(DEV)
    tr = Trainer(m, cfg, device=DEV, compute_dtype=dtype, graph_steps=graph_steps)
    return m, cfg, tr


def make_inputs(seed: int = BATCH_SEED):
    """(batch, meta) of druglamp_amd.synthetic.make_batch at batch 8: ragged lengths, graph input, bf16 LLM embeddings."""
    from druglamp_amd.synthetic import make_batch
    return make_batch(BATCH, DEV, seed=seed, with_graph=True, llm_dtype=torch.bfloat16)


def decoy_of(batch):
    """A second, equally valid batch of the same shapes, lengths and padding structure (the same meta and hints serve it) with
    other values everywhere: atom features and LLM embeddings halved (zero rows stay zero, virtual nodes stay identical),
    residue codes rotated within 1..25 (padding stays 0, a tiled sequence stays tiled)."""
    (h, adj), vp, y, xd, xp = batch
    h2 = h.clone()
    h2[:, :, :74] *= 0.5
    vp2 = torch.where(vp > 0, vp % 25 + 1, vp)
    return (h2, adj), vp2, 1.0 - y, xd * 0.5, xp * 0.5


def save_buffers(model) -> dict:
    return {k: b.detach().clone() for k, b in model.named_buffers()}


def restore_buffers(model, saved: dict) -> None:
    """Put the buffers (BatchNorm statistics and counters: all a forward + backward without an optimiser changes) back."""
    with torch.no_grad():
        for k, b in model.named_buffers():
            b.copy_(saved[k])


class SeedLog:
    """Wraps ops.next_seed for the length of a `with` block: `draws` lists (seed, the functional.py call site that drew it)."""

    def __init__(self):
        self.draws = []

    def __enter__(self):
        from druglamp_amd import ops
        self._ops, self._orig = ops, ops.next_seed

        def logged():
            v = self._orig()
            f = sys._getframe(1)
            line = f.f_lineno
            while f is not None and f.f_code.co_name.startswith("<"):       # (a draw inside a comprehension: the function around it)
                f = f.f_back
            code = f.f_code
            self.draws.append((v, "%s:%d" % (getattr(code, "co_qualname", code.co_name), line)))
            return v
        ops.next_seed = logged
        return self

    def __exit__(self, *exc):
        self._ops.next_seed = self._orig
        return False
