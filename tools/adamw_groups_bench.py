"""Cost of the grouped AdamW kernel against the plain one on the MI355X, at the trainer's own arena (14.03 M fp32 for the
DrugLAMP config) and with the chunk table real parameter groups give (no decay for vectors, encoders at a tenth of the lr).

dl_adamw_step and dl_adamw_step_groups ALTERNATE launch by launch in one process, on the same arena, gradient and moments;
after a warm-up of both, every launch is bracketed by a device-event pair and the medians of N >= 50 launches each are
compared.  The yardstick is dl_adamw_step in that same run: the grouped kernel moves 28.25 B per element against 28 B (under
1 % more), and may take up to 5 % longer — the rest of the margin is same-box spread.

    python tools/adamw_groups_bench.py [--launches 100] [--out profiles/param_groups_adamw.txt]
"""
import argparse, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from druglamp_amd import ops
from druglamp_amd.configs import get_cfg_defaults, load_yaml_into
from druglamp_amd.model import MInterface
from druglamp_amd.param_groups import ParamGroup
from druglamp_amd.trainer import Trainer

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=100)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "param_groups_adamw.txt"))
args = ap.parse_args()
assert args.launches >= 50
dev = torch.device("cuda:0")
torch.manual_seed(0); ops.manual_seed(1)
cfg = load_yaml_into(get_cfg_defaults(), "DrugLAMP")
model = MInterface("DrugLAMP", cfg).load_model(n_drug_feature=384, n_prot_feature=640).to(dev)
groups = [ParamGroup("no_decay", max_ndim=1, weight_decay=0.0),
          ParamGroup("encoders", match=("drug_extractor.*", "protein_extractor.*"), lr_scale=0.1)]
tr = Trainer(model, cfg, device=dev, compute_dtype=torch.bfloat16, param_groups=groups)
N = tr.flat.numel
arena, grads, m1, m2 = tr.flat.arena, torch.randn_like(tr.flat.arena) * 1e-3, tr.opt.exp_avg, tr.opt.exp_avg_sq
quads, tab = tr.param_groups.quad_group, tr.param_groups.group_tab
one = torch.zeros_like(quads)                              # every chunk in group 0: the table read without divergence
guard = torch.tensor([1.0, 1.0, 0.0, 0.0], device=dev)
kw = dict(lr=1e-6, step=3)
variants = [("dl_adamw_step", lambda: ops.adamw_step(arena, grads, m1, m2, **kw)),
            ("dl_adamw_step_groups, real table", lambda: ops.adamw_step_groups(arena, grads, m1, m2, quads, tab, **kw)),
            ("dl_adamw_step_groups, one group", lambda: ops.adamw_step_groups(arena, grads, m1, m2, one, tab, **kw)),
            ("dl_adamw_step_guarded", lambda: ops.adamw_step_guarded(arena, grads, m1, m2, guard, **kw)),
            ("dl_adamw_step_groups, real table, guard", lambda: ops.adamw_step_groups(arena, grads, m1, m2, quads, tab, guard=guard, **kw))]
for _ in range(10):                                        # warm-up of every variant
    for _, f in variants:
        f()
torch.cuda.synchronize()
events = {name: [] for name, _ in variants}
for _ in range(args.launches):                             # alternating: one launch of each, round after round
    for name, f in variants:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record()
        events[name].append((a, b))
torch.cuda.synchronize()
us = {name: sorted(a.elapsed_time(b) * 1e3 for a, b in ev) for name, ev in events.items()}
base = statistics.median(us["dl_adamw_step"])
segs = int((quads[1:] != quads[:-1]).sum()) + 1
lines = ["%s (%s), arena %d fp32, %d parameters, %d groups, %d segments of equal group id in the chunk table"
         % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, N, len(tr.flat.params), tab.shape[0], segs),
         "alternating launches, device events, %d launches each after a warm-up of 10 each; times in us" % args.launches]
for name, _ in variants:
    v = us[name]
    med = statistics.median(v)
    bytes_per = 28.25 if "groups" in name else 28.0
    lines.append("%-42s median %7.1f  min %7.1f  p90 %7.1f  (%.2f TB/s at %.2f B/element)  median / dl_adamw_step = %.4f"
                 % (name, med, v[0], v[int(0.9 * len(v))], bytes_per * N / med / 1e6, bytes_per, med / base))
ratio = statistics.median(us["dl_adamw_step_groups, real table"]) / base
lines.append("grouped / plain = %.4f (allowed: 1.05)%s" % (ratio, "" if ratio <= 1.05 else "  <-- a finding: explain before merging"))
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(text)
