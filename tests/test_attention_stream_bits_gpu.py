"""GPU: the streaming attention kernel (csrc/attention_stream.hip) reproduces, bit for bit, what the two kernels it was merged from
computed: tests/golden/attention_stream_bits.json holds the sha256 of the output rows of every case of
tests/attention_stream_cases.py, recorded on an MI355X from the commit before the merge."""
import pytest

import attention_stream_cases as A

pytestmark = pytest.mark.gpu


def test_streaming_attention_keeps_its_bits(device):
    gold = A.golden()
    assert (gold["width"], gold["fixed_batch"], gold["packed_lens"], gold["causal_lens"]) == (A.WIDTH, A.FIXED_BATCH, A.PACKED_LENS, A.CAUSAL_LENS)
    got = A.checksums(device)
    assert set(got) == set(gold["sha256"]) and len(got) == len(A.FIXED_T) + 3
    wrong = [name for name in got if got[name] != gold["sha256"][name]]
    assert not wrong, wrong
