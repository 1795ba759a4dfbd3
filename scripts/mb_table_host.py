"""Host cost of the Python table layer, per call, with kernels that take no time: a 64 K-slot table and 256-id batches — what is
left is the calling thread's work (the argument checks, the marshalling, the launches).  Per-table calls: `_DeviceTable.find`,
`upsert`, `find_or_insert`, `find_missed(sync=False)`, `assign`, and `apply_planned` over a prebuilt plan; per-variable calls:
`Variable.lookup` and `Variable.upsert` at 1 and 2 shards (both on one device).  One JSON line per call.
  python scripts/mb_table_host.py [--package DIR] [--tag NAME] [--run N]
--package: the directory that holds the `tfra_amd` package to measure (default: this tree's), so that two versions of the Python
layer can be run alternately against one built library."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--package", default=os.path.join(ROOT, "recommenders-addons_amd"))
ap.add_argument("--tag", default="tree")
ap.add_argument("--run", type=int, default=0)
ap.add_argument("--calls", type=int, default=2000)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package))
import torch
import tfra_amd.dynamic_embedding as de
from tfra_amd.dynamic_embedding.table_ops import SparsePlan

dev = torch.device("cuda", 0)
dim, B, K = 64, 256, args.calls
opt = de.optimizers.Adam(1e-3)
slots = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
table = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(dim), init_size=1 << 16, device="cuda:0", dim=dim,
                           name="mb_table_host", **slots)._table
# distinct ids per batch: find_or_insert and assign take unique keys
ids = [torch.randperm(1 << 14, device=dev)[:B].to(torch.int64).contiguous() for _ in range(64)]
vals = torch.randn((B, dim), device=dev)
grads = torch.randn((B, dim), device=dev) * 0.01
default_row = table._default_value.to(torch.float32)
params = opt.params(1)
plan = SparsePlan(dev, dim).build(ids[0])
variables = {n: de.Variable(dim=dim, devices=["cuda:0"] * n, initializer=0.5, name="mb_table_host_%d" % n, init_size=1 << 16)
             for n in (1, 2)}

CALLS = [
    ("table.find", lambda i: table.find(ids[i % 64])),
    ("table.upsert", lambda i: table.upsert(ids[i % 64], vals, unique_keys=True)),
    ("table.find_or_insert", lambda i: table.find_or_insert(ids[i % 64])),
    ("table.find_missed_nosync", lambda i: table.find_missed(ids[i % 64], sync=False)),
    ("table.assign", lambda i: table.assign(ids[i % 64], vals)),
    ("table.apply_planned", lambda i: table.apply_planned(params, plan, grads, default_row)),
]
for n, var in variables.items():
  CALLS.append(("variable.lookup_%dshard" % n, lambda i, var=var: var.lookup(ids[i % 64])))
  CALLS.append(("variable.upsert_%dshard" % n, lambda i, var=var: var.upsert(ids[i % 64], vals)))

for name, call in CALLS:
  for i in range(200):
    call(i)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for i in range(K):
    call(i)
  host = time.perf_counter() - t0
  torch.cuda.synchronize()
  total = time.perf_counter() - t0
  print(json.dumps({"bench": "mb_table_host", "package": args.tag, "run": args.run, "call": name, "calls": K,
                    "host_us_per_call": round(host / K * 1e6, 3), "total_us_per_call": round(total / K * 1e6, 3)}), flush=True)
