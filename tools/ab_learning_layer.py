#!/usr/bin/env python3
"""A/B of the Python learning layer between another tree of this repository (e.g. `git archive <parent>` extracted somewhere) and this one, on this
tree's built library (not a test):
  1. the seven train_*.py for three iterations / epochs in both trees with the same arguments: the JSON lines (seconds*, env_steps_per_s aside) and
     the --dump-params files must be equal, byte for byte;
  2. TRPO, PPO and SAC: two iterations with --snapshot in one tree, --load-policy plus one iteration in the other, both directions, against 1.;
  3. the host-side speed of five loops (tools/time_learning_loops.py), the two trees alternating, three processes each.
Every GPU process runs under its own `timeout`; the first failure ends the run.
usage: python tools/ab_learning_layer.py <other tree> <output directory>   ->  <output directory>/learning_layer_ab.txt, learning_layer_ab.jsonl"""
import filecmp
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.abspath(sys.argv[1])
OUT = os.path.abspath(sys.argv[2])
WORK = os.path.join(OUT, "ab_work")
os.makedirs(WORK, exist_ok=True)
ENV = dict(os.environ, CASSIE2D_LIB=os.path.join(ROOT, "cassierl_amd", "lib", "libcassie2d.so"))
LOG = open(os.path.join(OUT, "learning_layer_ab.txt"), "w")
TREES = {"parent": PARENT, "this": ROOT}


def say(s):
    print(s, flush=True)
    LOG.write(s + "\n")
    LOG.flush()


def run(tree, argv, limit=240):
    """One process in `tree`; returns its JSON lines without the timing entries.  A failure ends the job."""
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + argv, cwd=TREES[tree], env=ENV, capture_output=True, text=True)
    if p.returncode != 0:
        say("FAILED (%d) in %s: %s\n%s" % (p.returncode, tree, " ".join(argv), p.stderr[-3000:]))
        sys.exit(1)
    lines = []
    for l in p.stdout.splitlines():
        if l.startswith("{"):
            d = json.loads(l)
            if "loaded" in d:   # the load line: this must be the interrupted run continued, pool included
                if not d["sampler_restored"] or not d.get("pool_restored", True):
                    say("NOT RESTORED in %s: %s" % (tree, l))
                    sys.exit(1)
                continue
            lines.append({k: v for k, v in d.items() if not k.startswith("seconds") and k != "env_steps_per_s"})
    return lines


ON = ["--kind", "stand", "--control-mode", "Torque", "--horizon", "4"]
OFF = ["--kind", "stand", "--control-mode", "Torque", "--batch-size", "512", "--pool-size", "4096", "--min-pool-size", "1024", "--epoch-length", "6"]
CASES = [
    ("trpo32", "train_trpo.py", ["--envs-per-gpu", "512", "--hidden", "32,32"] + ON, "--n-itr"),
    ("trpo128", "train_trpo.py", ["--envs-per-gpu", "512", "--hidden", "128,128", "--init-std", "1.0"] + ON, "--n-itr"),
    ("vpg", "train_vpg.py", ["--envs-per-gpu", "512", "--log-kl"] + ON, "--n-itr"),
    ("ppo", "train_ppo.py", ["--envs-per-gpu", "512", "--epochs", "2"] + ON, "--n-itr"),
    ("ppo3d", "train_ppo.py", ["--envs-per-gpu", "256", "--env", "cassie3d", "--horizon", "4", "--epochs", "2"], "--n-itr"),
    ("es", "train_es.py", ["--envs-per-gpu", "512", "--kind", "stand", "--control-mode", "Torque", "--max-path-length", "8", "--table-size", "1048576"], "--n-itr"),
    ("ddpg", "train_ddpg.py", ["--envs-per-gpu", "512"] + OFF, "--n-epochs"),
    ("sac", "train_sac.py", ["--envs-per-gpu", "512"] + OFF, "--n-epochs"),
    ("td3", "train_td3.py", ["--envs-per-gpu", "512"] + OFF, "--n-epochs"),
]
bad = 0
say("# bit identity: three iterations / epochs in each tree; the JSON lines (seconds*, env_steps_per_s aside) and the --dump-params files")
full = {}
for name, script, args, nflag in CASES:
    res = {}
    for tree in TREES:
        dump = os.path.join(WORK, "%s_%s.npy" % (name, tree))
        argv = [script] + args + [nflag, "3", "--dump-params", dump]
        res[tree] = (run(tree, argv), dump)
        if tree == "this":
            say("python " + " ".join(argv[:-1]) + " <file>")
    same_lines = res["parent"][0] == res["this"][0] and len(res["this"][0]) == 3
    same_dump = filecmp.cmp(res["parent"][1], res["this"][1], shallow=False)
    bad += not (same_lines and same_dump)
    say("  %-8s lines %s   dump (%d bytes) %s" % (name, "equal" if same_lines else "DIFFERENT", os.path.getsize(res["this"][1]), "byte-equal" if same_dump else "DIFFERENT"))
    full[name] = res["this"]

say("# snapshots across the trees: two iterations with --snapshot in one tree, --load-policy plus one iteration in the other; against three uninterrupted")
for name in ("trpo32", "ppo", "sac"):
    _, script, args, nflag = [c for c in CASES if c[0] == name][0]
    for writer, reader in (("parent", "this"), ("this", "parent")):
        snap = os.path.join(WORK, "%s_%s.snap" % (name, writer))
        dump = os.path.join(WORK, "%s_resumed_in_%s.npy" % (name, reader))
        first = run(writer, [script] + args + [nflag, "2", "--snapshot", snap])
        last = run(reader, [script] + args + [nflag, "1", "--load-policy", snap, "--dump-params", dump])
        same_lines = first + last == full[name][0]
        same_dump = filecmp.cmp(dump, full[name][1], shallow=False)
        bad += not (same_lines and same_dump)
        say("  %-8s written by %-6s continued by %-6s lines %s   dump %s" % (name, writer, reader, "equal" if same_lines else "DIFFERENT",
                                                                          "byte-equal" if same_dump else "DIFFERENT"))
if bad:
    say("RESULT: %d comparisons DIFFER" % bad)
    sys.exit(2)
say("RESULT: every comparison equal")

say("# host-side speed: tools/time_learning_loops.py <tree>, parent and this tree alternating, three processes each; medians (min .. max)")
runs = {t: [] for t in TREES}
with open(os.path.join(OUT, "learning_layer_ab.jsonl"), "w") as f:
    for r in range(3):
        for tree in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            for d in run(tree, [os.path.join(ROOT, "tools", "time_learning_loops.py"), TREES[tree]], limit=420):
                d.update(tree=tree, run=r)
                f.write(json.dumps(d) + "\n")
                f.flush()
                runs[tree].append(d)
for loop in sorted({d["loop"] for d in runs["this"]}):
    v = {t: sorted(d["value"] for d in runs[t] if d["loop"] == loop) for t in TREES}
    med = {t: statistics.median(v[t]) for t in TREES}
    spread = v["parent"][-1] - v["parent"][0]
    say("  %-44s parent %.4g (%.4g .. %.4g)   this %.4g (%.4g .. %.4g)   diff %.3g, parent's spread %.3g: %s" % (
        loop, med["parent"], v["parent"][0], v["parent"][-1], med["this"], v["this"][0], v["this"][-1], med["this"] - med["parent"], spread,
        "inside" if abs(med["this"] - med["parent"]) <= spread else "OUTSIDE"))
