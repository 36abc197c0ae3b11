"""Every output buffer of the 8×8-tile engine's entry points, the halo deconv3 entry points and
the stand-alone GDN is bit-identical to the record in tests/golden/g11_engine_digests.json: the
library as it was before csrc/engine_fp32.hip was split by kernel family and its host launch
layer rewritten (tests/golden/gen_engine_digests.py lists the cases and makes the record)."""
import importlib.util
import json
import os

import pytest


def _generator(golden_dir):
    spec = importlib.util.spec_from_file_location(
        "gen_engine_digests", os.path.join(golden_dir, "gen_engine_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_engine_outputs_match_recorded_digests(device, golden_dir):
    gen = _generator(golden_dir)
    record = json.load(open(os.path.join(golden_dir, "g11_engine_digests.json")))
    assert (record["B"], record["H"], record["W"]) == (gen.B, gen.H, gen.W)
    assert tuple(record["channels"]) == gen.CHANNELS
    got = gen.digests(device)
    assert sorted(got) == sorted(record["digests"])
    differing = [key for key in sorted(got) if got[key] != record["digests"][key]]
    assert not differing, f"{len(differing)} of {len(got)} cases differ: {differing[:20]}"
