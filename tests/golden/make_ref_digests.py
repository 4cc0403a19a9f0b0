"""Records tests/golden/ref_digests.json: the unmodified reference's results (oracle/_ref, `make -C oracle ref`) for the cases
of tests/test_oracle_vs_ref.py and tests/test_regs.py, as SHA-256 digests (oracle_lib.RefRecord).  Where oracle/_ref is not
built, those tests hold the oracle to these records instead of skipping.  Run from the repository root, with oracle/_ref built:
    python tests/golden/make_ref_digests.py"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as ol  # noqa: E402

if not ol.have_ref():
    raise SystemExit("oracle/_ref is not built: make -C oracle ref")
env = dict(os.environ, CHAINDP_RECORD_REF_DIGESTS="1")
sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_oracle_vs_ref.py",
                          "tests/test_regs.py", "-k", "not straw_man"], cwd=ROOT, env=env))
