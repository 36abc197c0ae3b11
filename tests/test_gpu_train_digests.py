"""Every forward output and every gradient of a training step, and the entry points it launches in
order, are what tests/golden/g13_train_step_digests.json records, in all four precision modes at
N = 128 and 192: the tree as it was before the training chain moved into chain.py and each
backward was written once (tests/golden/gen_train_step_digests.py lists the cases and makes the
record)."""
import importlib.util
import json
import os

import pytest


def _generator(golden_dir):
    spec = importlib.util.spec_from_file_location(
        "gen_train_step_digests", os.path.join(golden_dir, "gen_train_step_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_train_steps_match_recorded_digests_and_launches(device, golden_dir):
    gen = _generator(golden_dir)
    record = json.load(open(os.path.join(golden_dir, "g13_train_step_digests.json")))
    assert (record["B"], record["H"], record["W"]) == (gen.B, gen.H, gen.W)
    assert tuple(record["channels"]) == gen.CHANNELS
    assert tuple(record["modes"]) == gen.MODES and tuple(record["cases"]) == gen.CASES
    got, launches = gen.digests(device)
    assert sorted(got) == sorted(record["digests"]) == sorted(record["launches"])
    assert len(got) == len(gen.MODES) * len(gen.CHANNELS) * len(gen.CASES)
    differing = []
    for key in sorted(got):
        want = record["digests"][key]
        assert sorted(got[key]) == sorted(want), key
        differing += [f"{key}:{name}" for name in sorted(want) if got[key][name] != want[name]]
    assert not differing, f"{len(differing)} digests differ: {differing[:20]}"
    for key in sorted(launches):
        assert launches[key] == record["launches"][key], key
