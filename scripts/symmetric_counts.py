#!/usr/bin/env python3
"""Record the symmetric scan's MMF_SYMMETRIC_DEBUG counters on the rows of tests/test_gpu_symmetric_records.py
(test_counters_against_the_entry_path) under the frozen threshold image, for both filings, as JSON on stdout:

    scripts/ab_build.sh entries -DMMF_SYM_RECORDS=0
    MMF_HG_LIBRARY=multimodal-fusion_amd/libmmf_hg_entries.so python scripts/symmetric_counts.py > tests/golden/symmetric_records_counts.json

That file holds the ENTRY path's counts (the build with -DMMF_SYM_RECORDS=0), which the test holds the record path to."""
import importlib.util
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("records_test", os.path.join(ROOT, "tests", "test_gpu_symmetric_records.py"))
t = importlib.util.module_from_spec(spec)
spec.loader.exec_module(t)
import multimodal_fusion_amd as mmf   # noqa: E402

out = {"library": os.path.basename(os.environ.get("MMF_HG_LIBRARY", "libmmf_hg.so"))}
for prune in (0, 1):
    with tempfile.TemporaryFile() as tmp:      # the library prints the line with fprintf(stderr)
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            t.records_call(mmf, "dup", 2348, 1, "cosine", "fast", live=0, prune=prune, debug=1)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        line = [l for l in tmp.read().decode().splitlines() if l.startswith("[mmf symmetric]")][0]
    m = re.search(r"received entries (\d+) \([\d.]+ per row, largest (\d+) of \d+\), fullest wave log (\d+) of (\d+), logged entries (\d+) .*records (\d+),", line)
    out["pruned" if prune else "complete"] = dict(received=int(m.group(1)), largest=int(m.group(2)), fullest=int(m.group(3)),
                                                  logged=int(m.group(5)), records=int(m.group(6)), line=line)
print(json.dumps(out, indent=1))
