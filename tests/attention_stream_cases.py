"""The cases whose output bits tests/golden/attention_stream_bits.json pins for the streaming attention kernel
(csrc/attention_stream.hip): seeded inputs, one launch each, the sha256 of the output bytes.  Not a test module.  The golden file was
recorded on an MI355X from the commit before the fixed-length and the packed kernels became one template, through entry points that
commit already had; tests/test_attention_stream_bits_gpu.py holds every later library to it.

The shapes are the smallest at which each branch of the kernel can still go wrong:
* fixed length (engine.op_attention, non-causal), width 128, batch 3 -- 6 or 18 work items on a grid padded to a multiple of 8, so
  some workgroups return at once: T = 289 (the first length on this route: a last chunk of 33 keys with one dead 32-key PV block, a
  last query block of one live row), 320 (whole chunks, no tail), 577 (a one-key last chunk), 1025 (the longest: nine query blocks);
* packed, without and with MPNet's bias (debug.op_attention_varlen[_bias]), width 128, max_t 512: one row, the edges of a 16-query
  tile, a 64-key chunk and a 128-query block, a second and a fourth query block, items whose later query blocks return early;
* packed causal (debug.op_attention_packed), width 128, max_t 288: every item above 128 rows (the streaming route), the diagonal
  inside a chunk and at a chunk edge, a third query block.

    python tests/attention_stream_cases.py        # on an MI355X: records the golden file from the library that is built
"""
import hashlib
import json
import os

import torch

WIDTH = 128
FIXED_BATCH = 3
FIXED_T = [289, 320, 577, 1025]
PACKED_MAX_T = 512
PACKED_LENS = [1, 16, 17, 63, 64, 65, 128, 129, 300, 512]
CAUSAL_MAX_T = 288
CAUSAL_LENS = [129, 130, 192, 193, 248, 288]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_stream_bits.json")


def qkv(rows, seed):
    """bf16 [rows, 3 WIDTH], queries pre-scaled: logits of a few units."""
    x = torch.randn(rows, 3 * WIDTH, generator=torch.Generator().manual_seed(seed))
    x[:, :WIDTH] *= 0.25
    return x.to(torch.bfloat16)


def row_start(lens):
    return torch.tensor([0] + list(lens)).cumsum(0).int()


def checksum(t):
    """sha256 of the tensor's bytes (CPU copy, contiguous)."""
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def checksums(device):
    """{case name: sha256 of the output rows}, one launch per case."""
    import mpnet_ref as M
    from knowledge_enhanced_multimodal_retrieval_amd import debug, engine, hf_checkpoint
    sums = {}
    for t in FIXED_T:
        sums[f"fixed_t{t}"] = checksum(engine.op_attention(qkv(FIXED_BATCH * t, 1000 + t).to(device), FIXED_BATCH, t, WIDTH, False))
    rs = row_start(PACKED_LENS)
    x, rsd = qkv(int(rs[-1]), 2000).to(device), rs.to(device)
    table = hf_checkpoint.bias_by_distance(M.bias_weight(WIDTH // 64)).to(device)
    sums["packed"] = checksum(debug.op_attention_varlen(x, rsd, PACKED_MAX_T, WIDTH))
    sums["packed_bias"] = checksum(debug.op_attention_varlen_bias(x, rsd, table, PACKED_MAX_T, WIDTH))
    rs = row_start(CAUSAL_LENS)
    sums["packed_causal"] = checksum(debug.op_attention_packed(qkv(int(rs[-1]), 3000).to(device), rs.to(device), CAUSAL_MAX_T, WIDTH))
    return sums


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record = {"what": "sha256 of the output rows (bf16 bytes) of tests/attention_stream_cases.py checksums(), recorded on an MI355X from "
                      "the commit before csrc/attention_long.hip and csrc/attention_varlen.hip became csrc/attention_stream.hip",
              "width": WIDTH, "fixed_batch": FIXED_BATCH, "packed_lens": PACKED_LENS, "causal_lens": CAUSAL_LENS,
              "sha256": checksums(torch.device("cuda:0"))}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record["sha256"], indent=1))
