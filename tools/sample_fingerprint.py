"""SHA-256 of every output of the case list of tests/sample_routes.py (the spectra, tsdr_fft_c2c_d, the demodulators and the
autocorrelations on real f32, ComplexF32, sc16, sc8 and uc8 input) on seeded inputs: a host-side change leaves every digest as it
was.  Welch's summation grouping follows the device's CU count, so two runs compare on ONE machine only:
    TSDR_HIP_LIB=<the other build's libtempest_hip.so> python tools/sample_fingerprint.py before.json
    python tools/sample_fingerprint.py after.json  &&  cmp before.json after.json"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sample_routes as S  # noqa: E402
from tempest_loader import load_package  # noqa: E402

ctx = load_package().Context(0)
digests = {}
for name, prepare in S.cases():
    h = hashlib.sha256()
    for a in S.run(ctx, prepare):
        h.update(a.tobytes())
    digests[name] = h.hexdigest()
text = json.dumps({"device": ctx.device_info()["name"], "cu_count": ctx.device_info()["cu_count"], "sha256": digests}, indent=0, sort_keys=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
print(f"{len(digests)} cases, digest of digests {hashlib.sha256(text.encode()).hexdigest()[:16]}")
