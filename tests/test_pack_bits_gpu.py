"""k_pack_bits (uint8 [batch][len] -> bit planes) fetches each codeword's 16-byte stretches with aligned dword loads, whatever
the alignment of the row or of the caller's pointer, and reads no byte outside the input.  Here every call decodes random
inputs for two min-sum iterations and is held to the float32 oracle, so a mispacked bit surfaces in `bits` (received mode:
the output is the input XOR the decisions; syndrome mode: every syndrome bit moves the decisions of its row's columns).
Graphs [Hin | I] with n = 0, 1, 10 and 15 (mod 16), one with m below 16 and one with n below 16; batch 1, 63, 64, 65, 129;
received words (n bytes per codeword) and syndromes (m bytes); host arrays, and device pointers at byte offsets 0 ... 3 into
a larger tensor whose other bytes are 0xFF.  The path is pinned to the 64-codeword-tile kernels."""
import importlib

import numpy as np
import pytest

S = importlib.import_module("sca-ldpc_amd")
bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")

pytestmark = pytest.mark.gpu
MAX_ITER = 2
BATCHES = (1, 63, 64, 65, 129)
# (N, W, R): n = N + R columns, m = R rows
GRAPHS = {"n128": (90, 5, 38), "n129": (91, 5, 38), "n138": (100, 5, 38), "n143": (105, 5, 38), "n47_m7": (40, 3, 7),
          "n13_m4": (9, 2, 4)}  # fmt: skip


def graph(name):
    N, W, R = GRAPHS[name]
    rng = np.random.RandomState(len(name) + N)
    sup = np.sort(rng.choice(N, W, replace=False))
    H = S.codes.hqc_check_graph(sup, N, rng.permutation(N)[:R]).with_identity()
    assert (H.n, H.m) == (N + R, R)
    return H, np.concatenate([np.full(N, 0.05), np.full(R, 0.1)]), rng


def device_call(torch, dec, x, kind, n, offset):
    """The input at `offset` bytes into a tensor of 0xFF; returns the decisions."""
    batch = x.shape[0]
    buf = torch.full((offset + x.size + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[offset : offset + x.size] = torch.from_numpy(x.reshape(-1)).cuda()
    d_out = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dec.decode_batch_device(buf.data_ptr() + offset, kind, batch, d_out.data_ptr(), max_iter=MAX_ITER, early_exit=False,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_packed_inputs_decode_as_the_oracle(scaldpc, oracle, name):
    import torch

    H, probs, rng = graph(name)
    assert (H.n % 16, H.m < 16, H.n < 16) == {"n128": (0, False, False), "n129": (1, False, False), "n138": (10, False, False),
                                               "n143": (15, False, False), "n47_m7": (15, True, False),
                                               "n13_m4": (13, True, True)}[name]  # fmt: skip
    dec = bp.bp_decoder(H, max_iter=MAX_ITER, bp_method="min_sum", channel_probs=probs)
    dec.configure(path="stream")
    for batch in BATCHES:
        for kind, length in ((lib.IN_RECEIVED, H.n), (lib.IN_SYNDROME, H.m)):
            x = (rng.rand(batch, length) < 0.3).astype(np.uint8)
            ref = oracle.bp_decode_batch(H, probs, x, kind, MAX_ITER, "min_sum", dtype="f32", threads=2, early_exit=False)
            got = dec.decode_batch(x, max_iter=MAX_ITER, early_exit=False)
            assert (got["bits"] == ref["bits"]).all(), (name, batch, kind, "host")
            for offset in range(4):
                bits = device_call(torch, dec, x, kind, H.n, offset)
                assert (bits == ref["bits"]).all(), (name, batch, kind, offset)
    dec.close()


def test_only_bit_0_counts(scaldpc, oracle):
    """Arbitrary bytes: a codeword's bit is bit 0 of its byte, from host arrays and from every device offset."""
    import torch

    H, probs, rng = graph("n143")
    dec = bp.bp_decoder(H, max_iter=MAX_ITER, bp_method="min_sum", channel_probs=probs)
    dec.configure(path="stream")
    for kind, length in ((lib.IN_RECEIVED, H.n), (lib.IN_SYNDROME, H.m)):
        x = rng.randint(0, 256, size=(65, length)).astype(np.uint8)
        x[:, ::7] |= 0xFE  # (bytes 0xFE and 0xFF among them)
        ref = oracle.bp_decode_batch(H, probs, x & 1, kind, MAX_ITER, "min_sum", dtype="f32", threads=2, early_exit=False)
        assert (dec.decode_batch(x, max_iter=MAX_ITER, early_exit=False)["bits"] == ref["bits"]).all(), (kind, "host")
        for offset in range(4):
            assert (device_call(torch, dec, x, kind, H.n, offset) == ref["bits"]).all(), (kind, offset)
    dec.close()
