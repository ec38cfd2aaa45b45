"""The committed csrc/eval_asm.inc is what tools/gen_eval_asm.py generates (the build does not run the generator)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_reproduces_committed_eval_asm(tmp_path):
    out = tmp_path / "eval_asm.inc"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_eval_asm.py"), str(out)],
                          stdout=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "gadget-2.0.7-ngravs_amd", "csrc", "eval_asm.inc"), "rb") as f:
        committed = f.read()
    assert out.read_bytes() == committed
