"""tools/tablelib.py -- what the *_table.py tools (attn_decode, rope_append, rmsnorm, moe_gate) share: the two clocks of their tables and
the device-side paged KV cache of the first two.  torch is imported inside the functions: --build-only runs need no device.
Two clocks, the columns alternated in one process on warm buffers, median of REPEATS:
  graph   `calls` calls captured into one hipGraph, REPLAYS replays between two events: device time, no host launch cost;
  eager   `calls` calls between two events, launch gaps included."""
import csv
import ctypes
import os
import statistics
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS, CALLS, REPLAYS = 5, 20, 3


def attn_shapes():
    """the rows (q_heads, kv_heads, head_dim, page_size) of datasets/attn_shapes.csv"""
    with open(os.path.join(ROOT, "datasets", "attn_shapes.csv")) as fh:
        rows = [r for r in csv.reader(l for l in fh if not l.startswith("#"))]
    return [tuple(int(x) for x in r) for r in rows[1:]]


def probe_lib(name, source, define):
    """tools/probes/lib<name>.so: the translation unit tools/probes/<source> alone with -D<define>; built when it is not there"""
    path = os.path.join(ROOT, "tools", "probes", f"lib{name}.so")
    if not os.path.exists(path):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-D" + define,
                        os.path.join(ROOT, "tools", "probes", source), "-o", path], check=True)
    return ctypes.CDLL(path)


def timed(run):
    """us per call of run(), which returns how many calls it made"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    n = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def clocks(fn, calls=CALLS):
    """(graph, eager): two callables, each returns us per call of fn"""
    import torch
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()

    def graph():
        for _ in range(REPLAYS):
            g.replay()
        return calls * REPLAYS

    def eager():
        for _ in range(calls):
            fn()
        return calls
    return (lambda: timed(graph)), (lambda: timed(eager))


def medians(cols):
    """cols: name -> clock.  REPEATS rounds over all columns in turn; returns (name -> median, name -> every run)"""
    runs = {k: [] for k in cols}
    for _ in range(REPEATS):
        for k, f in cols.items():
            runs[k].append(f())
    return {k: statistics.median(v) for k, v in runs.items()}, runs


def paged_cache(gen, dev, seqs, max_pages, page_size, kv_heads, head_dim, normal):
    """(K, V, block_table) on dev: bf16 caches [seqs * max_pages][page_size][kv_heads][head_dim] -- N(0, 1) from gen when `normal`, else zeros
    -- and the int32 table [seqs][max_pages], the pages scattered by a random permutation from gen"""
    import torch
    shape = (seqs * max_pages, page_size, kv_heads, head_dim)
    if normal:
        K, V = (torch.empty(shape, device=dev, dtype=torch.bfloat16).normal_(generator=gen) for _ in range(2))
    else:
        K, V = (torch.zeros(shape, device=dev, dtype=torch.bfloat16) for _ in range(2))
    return K, V, torch.randperm(shape[0], generator=gen, device=dev).to(torch.int32).view(seqs, max_pages)
