"""The launch list of the device-stepped decodes is pinned: the library entry points of one whole "device" call, name by name and in
order, for the TTS and ASR cases of tools/decode_step_calls.py on the tiny golden models, against tests/golden/decode_step_calls.json
-- recorded by that tool on the tree before step_program.py existed (three copies of the layer sequence, two of the builders and the
loop).  Whole call by whole call, so the set-up launches are pinned with the steps."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded(cuda):
    spec = importlib.util.spec_from_file_location("decode_step_calls", os.path.join(ROOT, "tools", "decode_step_calls.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.record(cuda)


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(ROOT, "tests", "golden", "decode_step_calls.json")) as f:
        return json.load(f)


def test_the_cases_are_the_pinned_ones(recorded, pinned):
    assert sorted(recorded) == sorted(pinned) and len(pinned) == 10
    assert sum(k.startswith("tts ") for k in pinned) == 6 and sum(k.startswith("asr ") for k in pinned) == 4


@pytest.mark.parametrize("case", ["tts pre-ln spk need_attn=False", "tts pre-ln spk need_attn=True", "tts pre-ln no-spk need_attn=False",
                                  "tts pre-ln no-spk need_attn=True", "tts post-ln spk need_attn=False", "tts post-ln spk need_attn=True",
                                  "asr plain", "asr ctc", "asr lm", "asr ctc lm"])
def test_library_calls_are_the_pinned_ones(recorded, pinned, case):
    got, want = recorded[case], pinned[case]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"{len(got)} calls against {len(want)}; first difference at call {first}: {got[first:first + 3]} != {want[first:first + 3]}"
    assert "st5_gemm_skinny" in want
