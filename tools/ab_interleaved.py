"""Developer aid: A/B of library builds on one box, interleaved rounds (cdna guide rule 24).
Usage: python tools/ab_interleaved.py [--rounds R] [--shapes c2,c3,s2048,...] lib_a.so lib_b.so ...   ("tree" = the in-tree library)
Each round runs every build in a fresh child process with FA_FWD_LIB set to that build (the compiled binding calls the
library it was loaded with, so builds cannot be swapped inside one process); prints median / best TFLOP/s per build and
checks that the builds agree on the last round's outputs."""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

SHAPES = {  # name: (b, s, h, d, causal, dtype)
    "c2": (4, 8192, 16, 128, False), "c3": (4, 16384, 16, 128, True), "s512": (32, 512, 16, 128, False),
    "s1024": (16, 1024, 16, 128, False), "s2048": (8, 2048, 16, 128, False), "s2048c": (8, 2048, 16, 128, True),
    "s4096": (4, 4096, 16, 128, False), "d64": (2, 8192, 32, 64, False), "d64c": (2, 8192, 32, 64, True),
    "d96": (2, 8192, 21, 96, False), "d256": (2, 8192, 8, 256, False), "d256c": (2, 8192, 8, 256, True),
    "d192": (2, 8192, 10, 192, False), "d160": (2, 8192, 12, 160, False),
    "c5": (4, 8192, 16, 128, False), "c5c": (4, 8192, 16, 128, True),   # fp8 e4m3 inputs (FA3 surface)
}


def child(sh, outfile):
    """One build (FA_FWD_LIB, set by the parent): warm up, print the median of 20 timed calls (ms), save the outputs."""
    import flash_attention_annotated_amd as fa
    b, s, h, d, causal = SHAPES[sh]
    torch.manual_seed(0)
    q, k, v = (torch.randn(b, s, h, d, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    if sh.startswith("c5"):
        from flash_attention_annotated_amd import hopper_interface as fa3
        q, k, v = (x.to(torch.float8_e4m3fn) for x in (q, k, v))
        run = lambda: fa3.flash_attn_func(q, k, v, causal=causal, return_attn_probs=True)
    else:
        run = lambda: fa.flash_attn_func(q, k, v, causal=causal, return_attn_probs=True)
    for _ in range(10): run()   # warm up (clock, caches, lazy module load)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for a, e in ev:
        a.record(); r = run(); e.record()
    torch.cuda.synchronize()
    torch.save((r[0].float().cpu(), r[1].float().cpu()), outfile)
    print(sorted(a.elapsed_time(e) for a, e in ev)[len(ev) // 2])


if len(sys.argv) == 4 and sys.argv[1] == "--child":
    child(sys.argv[2], sys.argv[3])
    sys.exit(0)

args = sys.argv[1:]
rounds, shapes = 5, ["c2"]
if "--rounds" in args:
    i = args.index("--rounds"); rounds = int(args[i + 1]); del args[i:i + 2]
if "--shapes" in args:
    i = args.index("--shapes"); shapes = args[i + 1].split(","); del args[i:i + 2]
libs = args or ["tree"]
tmp = tempfile.mkdtemp()


def run_child(sh, n):
    env = dict(os.environ)
    env.pop("FA_FWD_LIB", None)
    if n != "tree":
        env["FA_FWD_LIB"] = os.path.abspath(n)
    outfile = os.path.join(tmp, f"{libs.index(n)}.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", sh, outfile], env=env, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f"{sh} {n}: child failed ({r.returncode}):\n{r.stderr}")
    return float(r.stdout.split()[-1])


for sh in shapes:
    b, s, h, d, causal = SHAPES[sh]
    fl = 4 * b * h * s * s * d / (2 if causal else 1)
    res = {n: [] for n in libs}
    for r in range(rounds):
        for n in libs:
            res[n].append(run_child(sh, n))
    outs = {n: torch.load(os.path.join(tmp, f"{libs.index(n)}.pt")) for n in libs}
    for n in libs[1:]:   # the builds must agree (schedule variants are bit-identical by construction)
        do = (outs[n][0] - outs[libs[0]][0]).abs().max().item()
        dl = (outs[n][1] - outs[libs[0]][1]).abs().max().item()
        if do != 0 or dl != 0:
            print(f"   !! {os.path.basename(n)} differs from {os.path.basename(libs[0])}: out {do:.3e} lse {dl:.3e}", flush=True)
    for n in libs:
        ms = sorted(res[n])
        print(f"{sh:7s} {os.path.basename(n):28s} median {fl / ms[len(ms) // 2] / 1e9:7.1f}  best {fl / ms[0] / 1e9:7.1f} TFLOP/s   ({ms[len(ms) // 2]:.4f} ms)", flush=True)
