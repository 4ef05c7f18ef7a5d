"""Every engine handle packs what it packed before the front-ends were rebased onto EngineModel (safe_denoiser_amd/_model.py):
tests/golden/pack_digests.json holds, per handle of tests_support/pack_cases.py, the sha256 of pack_state_dict(synthetic_state_dict),
of the manifest and of the source shapes, taken at the commit before that change (tests/golden/make_pack_digests.py), and on the
GPU the sha256 of the manifest regions of load_synthetic_on_device -- the weights the benchmark runs on.  The `device` section holds the
handles whose value could be recorded on an MI355X at that earlier commit (make_pack_digests.py --device there); a handle without a
record is compared on the upload alone, never against a value taken from later code."""
import json
import os

import pytest
import torch

from tests_support import pack_cases as PC

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_digests.json")) as _f:
    GOLD = json.load(_f)


def test_the_fixture_covers_every_handle():
    assert GOLD["seed"] == PC.SEED and set(GOLD["host"]) == set(PC.CASES) and set(GOLD["device"]) <= set(PC.CASES)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_packed_bytes_manifest_and_shapes_are_the_recorded_ones(name):
    make, alias = PC.CASES[name]
    m, want = make(), GOLD["host"][name]
    assert int(m.weight_bytes) == want["weight_bytes"]
    assert PC.manifest_digest(m) == want["manifest"]
    assert PC.shapes_digest(m) == want["shapes"]
    sd = m.synthetic_state_dict(PC.SEED)
    buf = m.pack_state_dict(sd)
    assert buf.dtype == torch.uint8 and buf.device.type == "cpu" and buf.numel() == m.weight_bytes
    assert PC.sha(buf) == want["packed"]
    other = alias(sd)
    assert set(other) != set(sd)
    assert PC.sha(m.pack_state_dict(other)) == want["packed"]                  # the prefixed / aliased / on-disk key forms
    gone = next(p["name"] for p in reversed(m.manifest) if "quant_conv" not in p["name"])     # (a mixer may be the identity's)
    with pytest.raises(KeyError):
        m.pack_state_dict({k: v for k, v in sd.items() if k != gone})


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PC.CASES))
def test_upload_equals_the_host_pack_and_synthetic_device_weights_are_the_recorded_ones(name):
    make, _ = PC.CASES[name]
    m = make()
    sd = m.synthetic_state_dict(PC.SEED)
    host = m.pack_state_dict(sd)
    dev = m.load_state_dict(sd)._weights
    assert dev.is_cuda and dev.numel() == host.numel()
    for p, a, b in zip([q for q in m.manifest if q["kind"] != PC.P_GLU_GATE], PC.regions(m, dev.cpu()), PC.regions(m, host)):
        assert torch.equal(a, b), p["name"]
    if name in GOLD["device"]:                                                  # (recorded on an MI355X before the change)
        m.load_synthetic_on_device(PC.SEED)
        assert PC.regions_digest(m, m._weights) == GOLD["device"][name]
