"""Every output buffer (h3, fp32, x6, pre-activation) of the h3 engine's GDN / IGDN layers is
bit-identical to the record in tests/golden/g12_h3_epilogue_digests.json: the library as it was
while the epilogue's channel contraction still ran in two passes over the output tiles, each
splitting every k-block's x² again (tests/golden/gen_h3_epilogue_digests.py lists the cases —
ragged and full tiles, 8- and 16-row workgroups, integer and real input, both h3 output layouts,
all-zero and near-zero pixels — and makes the record)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu


def _generator(golden_dir):
    spec = importlib.util.spec_from_file_location(
        "gen_h3_epilogue_digests", os.path.join(golden_dir, "gen_h3_epilogue_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("N", [128, 192])
@pytest.mark.parametrize("group", ["conv1", "conv2", "deconv"])
def test_epilogue_outputs_match_recorded_digests(device, golden_dir, group, N):
    gen = _generator(golden_dir)
    record = json.load(open(os.path.join(golden_dir, "g12_h3_epilogue_digests.json")))
    assert tuple(record["channels"]) == gen.CHANNELS and group in gen.GROUPS
    want = {k: v for k, v in record["digests"].items()
            if k.startswith(f"N{N}/{group}.") or k == f"N{N}/{group}"}
    got = gen.digests(device, N, group)
    assert want and sorted(got) == sorted(want)
    differing = [f"{key}[{i}]" for key in sorted(got) for i in sorted(got[key])
                 if got[key][i] != want[key].get(i)]
    assert not differing, f"{len(differing)} buffers differ: {differing[:20]}"
