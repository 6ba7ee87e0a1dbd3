"""GPU tests of the batched encoder (csrc/encode_kernels.hpp): the device
path against the host encoder bit for bit, the DNA code against its 272
reference codewords, a full encode -> channel -> decode -> extract round trip
on a code that has no fixture codewords, and generated codewords as the
synthetic channel's input."""
import numpy as np
import pytest

import gf2_ref

pytestmark = pytest.mark.gpu


# partial tiles, K and M off word and byte alignment, rank deficiency; "tall":
# M above the 8192 rows whose parities the dense kernel keeps in LDS
@pytest.mark.parametrize("name", ["rs_5_16_4", "r37x100", "r65x129", "tall"])
def test_device_equals_host(gpu, name):
    enc = gf2_ref.small_graph(gpu, name).encoder()
    m = (np.random.default_rng(4).random((130, enc.K)) < 0.5).astype(np.uint8)
    want = enc.encode_host(m)
    for B in (1, 63, 64, 65, 130):
        assert np.array_equal(enc.encode(m[:B]), want[:B]), B
    assert np.array_equal(enc.encode(m[7]), want[7])  # a 1-D array is one message


def test_dna_code_on_the_device(gpu, G, codewords):
    enc = G.encoder()
    msg = np.ascontiguousarray(codewords[:, enc.info_pos])
    assert np.array_equal(enc.encode(msg), codewords)  # four full tiles + 16 lanes
    # device buffers: an engine's stream (asynchronous), and the library's own
    B = 272
    d_msg, d_a, d_b = (gpu.DeviceBuffer(0, n) for n in (msg.nbytes, B * G.N, B * G.N))
    d_msg.upload(msg)
    eng = gpu.Engine(G, 0, "bp", chunk=64)
    enc.encode_device(d_msg, B, d_a, device=0, stream=eng.stream)
    eng.sync()
    enc.encode_device(d_msg, B, d_b, device=0, stream=None)
    a = d_a.download(np.empty((B, G.N), np.uint8))
    b = d_b.download(np.empty((B, G.N), np.uint8))
    assert np.array_equal(a, codewords) and np.array_equal(b, codewords)
    with pytest.raises(ValueError):
        enc.encode_device(d_msg, B + 1, d_a)
    eng.close()


def test_round_trip_rs_7_72_6(gpu, oracle_mod, tmp_path):
    """Row degree 72 with column degree 6: encode on the device, one bit
    error per codeword, BP decode on the device returns what was stored."""
    import synth
    R = gpu.Graph.rs_ldpc(7, 72, 6)
    assert (R.dc, R.dv, R.N) == (72, 6, 9216)
    enc = R.encoder()
    B = 130
    msg = synth.random_messages(enc.K, 0, B, seed=7)
    cw = enc.encode(msg)
    assert np.array_equal(cw, enc.encode_host(msg))
    rx = cw.copy()
    b = np.arange(B)
    rx[b, (977 * b) % R.N] ^= 1  # exactly one flipped bit per codeword
    assert ((rx != cw).sum(axis=1) == 1).all()
    llr = np.where(rx == 1, -synth.LLR_UNIT, synth.LLR_UNIT)  # +-ln 49
    # precondition: the oracle decodes all of them to the transmitted words
    p = str(tmp_path / "rs_7_72_6.pchk")
    R.save_pchk(p)
    rh, _, rit, rv = oracle_mod.OracleGraph(p).decode_batch(llr, 10, threads=8, want_post=False)
    assert np.array_equal(rh, cw) and rv.all()
    h, _, it, v = R.decode(llr, max_iter=10, algo="bp", post=None)
    assert np.array_equal(h, cw)
    assert np.array_equal(enc.extract(h), msg)
    assert np.array_equal(it, rit) and np.array_equal(v, rv.astype(bool))


def test_generated_codewords_feed_the_channel_generator(gpu):
    import synth
    R = gpu.Graph.rs_ldpc(5, 16, 4)
    enc = R.encoder()
    n_cw = 130
    cw = synth.random_codewords(enc, 0, n_cw, seed=3, device=0)
    assert np.array_equal(cw, synth.random_codewords(enc, 0, n_cw, seed=3))
    d_cw = gpu.DeviceBuffer(0, cw.nbytes)
    d_cw.upload(cw)
    B = 200  # wraps around the 130 codewords
    d_out = gpu.DeviceBuffer(0, B * R.N)
    eng = gpu.Engine(R, 0, "bp", chunk=64)
    eng.gen_bsc_codes(d_out.at(0), 0, B, d_cw.at(0), n_cw, 11, 0.0)
    eng.sync()
    codes = d_out.download(np.empty((B, R.N), np.int8))
    assert np.array_equal(codes, 1 - 2 * cw[np.arange(B) % n_cw].astype(np.int8))
    eng.close()
