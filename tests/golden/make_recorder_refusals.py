"""Generates tests/golden/recorder_refusals.json: what tools/run_sweep.py answers to every command line that asks for a
recording of the production run (--error-bars, --hist, --corr, --shape) it must refuse, recorded from the commit BEFORE the
four options became one value (polymer_stats_amd/_host.py: Recording), so that tests/test_host.py can hold the hosts to the
exact words.  The rows are the command lines of the refusal tests of tests/test_blocking_cpu.py, test_hist_cpu.py,
test_corr_cpu.py and test_shape_cpu.py, the six pairings of two of the four flags and two command lines with three.  Exactly
one refusal applies to a row, except where several flags are given: there the line is the rivals' sentence.  Each row:

  argv     what follows the work directory on the tool's command line (--dry-run first: no GPU is needed)
  status   the exit status
  line     the refusal, the one line the tool leaves on stderr

Run:  python tests/golden/make_recorder_refusals.py [CHECKOUT]   (runs CHECKOUT's tool, default: this tree's, and rewrites
      the JSON next to this file)
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

EB = ["--axis", "E0=1,2", "--error-bars", "64"]
AXES = ["--axis", "n=8", "--axis", "Fz=0,1"]
H, C, S = ["--hist", "r3:-8:8:32"], ["--corr", "5"], ["--shape", "z:6:8"]
T3, T6 = ["--", "--num-steps", "3000", "--stepout", "100"], ["--", "--num-steps", "6400", "--stepout", "100"]
ROWS = [
    # tests/test_blocking_cpu.py
    EB + ["--csv"], EB + ["--gpus", "2"], EB + ["--", "--devices", "0,1"], EB + ["--", "--num-inits", "2"],
    EB + ["--", "--umbrella-sampling"], EB + ["--", "--numeric-type", "float128"],
    EB + ["--main", "mcmc_clustering_eap_chain", "--", "--umbrella-sampling"],
    EB + ["--main", "mcmc_clustering_eap_chain_2d", "--", "--numeric-type", "big"],
    ["--axis", "E0=1,2", "--error-bars", "16"], EB + ["--", "--num-steps", "63"],
    # tests/test_hist_cpu.py
    AXES + H + ["--csv"] + T3, AXES + H + ["--gpus", "2"] + T3, AXES + H + ["--error-bars", "32"] + T3,
    AXES + H + T3 + ["--umbrella-sampling"], AXES + H + T3 + ["--num-inits", "2"], AXES + ["--hist", "r4:-8:8:32"] + T3,
    AXES + ["--hist", "r3:8:-8:32"] + T3, AXES + H + T3 + ["--stepout", "5000"],
    # tests/test_corr_cpu.py
    AXES + C + ["--csv"] + T6, AXES + C + ["--gpus", "2"] + T6, AXES + C + ["--error-bars", "32"] + T6, AXES + C + H + T6,
    AXES + C + T6 + ["--umbrella-sampling"], AXES + C + T6 + ["--num-inits", "2"], AXES + ["--corr", "5:nn,xx"] + T6,
    AXES + ["--corr", "8"] + T6, AXES + C + T6 + ["--stepout", "5000"],
    # tests/test_shape_cpu.py
    AXES + S + ["--csv"] + T6, AXES + S + ["--gpus", "2"] + T6, AXES + S + ["--error-bars", "32"] + T6, AXES + S + H + T6,
    AXES + S + C + T6, AXES + ["--shape"] + T6 + ["--umbrella-sampling"], AXES + S + T6 + ["--num-inits", "2"],
    AXES + ["--shape", "w:6:8"] + T6, AXES + ["--shape", "z:6"] + T6, AXES + ["--shape", "z:6:0"] + T6,
    AXES + ["--shape", "z:6:300,x:6:300"] + T6, AXES + ["--shape", "z:20000:4"] + T6, AXES + S + T6 + ["--stepout", "5000"],
    ["--main", "mcmc_clustering_eap_chain_2d", "--axis", "n=8", "--shape", "y:6:8"] + T6,
    # the six pairings of two flags, earlier flag first (the tests above name them the other way round), then three at once
    AXES + ["--error-bars", "32"] + H + T6, AXES + ["--error-bars", "32"] + C + T6, AXES + ["--error-bars", "32"] + S + T6,
    AXES + H + C + T6, AXES + H + S + T6, AXES + C + S + T6,
    AXES + ["--error-bars", "32"] + H + C + T6, AXES + H + C + S + T6,
]


def rows(checkout: str) -> list:
    tool = os.path.join(checkout, "tools", "run_sweep.py")
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for argv in ROWS:
            argv = ["--dry-run"] + argv
            r = subprocess.run([sys.executable, tool, os.path.join(tmp, "w")] + argv, capture_output=True, text=True)
            lines = r.stderr.strip().split("\n")
            assert r.returncode != 0 and len(lines) == 1 and not os.path.exists(os.path.join(tmp, "w")), (argv, r.returncode, r.stderr)
            out.append(dict(argv=argv, status=r.returncode, line=lines[0]))
    return out


if __name__ == "__main__":
    checkout = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
    with open(os.path.join(HERE, "recorder_refusals.json"), "w") as f:
        f.write("[\n" + ",\n".join("  " + json.dumps(r, ensure_ascii=False) for r in rows(checkout)) + "\n]\n")
