"""MI355X: every flow of generate_flow_cases.FLOWS through generate_indices.generate() -- whole file and --extend, with and without
the beam steps, --spill and --audit -- writes the bytes and returns the statistics recorded in tests/golden/f14_generate_flows.json
by tools/record_generate_flows.py, before the two flows shared one finishing pipeline.  The end-to-end tests beside this one
(test_gpu_finish, _extend, _spill, _beam_finish, _extend_beam) say that these tuples are the right ones; this file says that they,
and every statistic, stay what they were."""
import json
import os

import pytest

import generate_flow_cases as gfc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLD, "f14_generate_flows.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def setup(hip, tmp_path_factory):
    """the checkpoints and the --extend bases, each built once"""
    from lcrec_amd import generate_indices as gen
    return gfc.Setup(gen, tmp_path_factory.mktemp("flows"))


def test_the_fixture_holds_every_flow_and_has_work_for_every_step(recorded):
    assert sorted(recorded["flows"]) == sorted(gfc.FLOW_IDS)
    stats = [json.loads(f["stats"]) for f in recorded["flows"].values()]
    assert any(s.get("spill_moved", 0) > 0 for s in stats) and any(s.get("finish_beam_moved", 0) > 0 for s in stats)
    assert any(s.get("extend_beam_moved", 0) > 0 for s in stats)
    assert any("extend_beam_width" in s and s["extend_moved"] > 0 for s in stats)


@pytest.mark.parametrize("flow", gfc.FLOWS, ids=gfc.FLOW_IDS)
def test_generate_flow(setup, recorded, flow):
    want = recorded["flows"][flow["id"]]
    got = setup.run(flow)
    where = f"{flow['id']}: not as recorded ({recorded['commit'][:12]}, {recorded['device']})"
    assert got["stats"] == want["stats"], where
    assert got["sha256"] == want["sha256"], where
