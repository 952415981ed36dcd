"""The HIP sampling kernel (csrc/kernels/sample.hip) against the fp64 oracle of tests/sampling_oracles.py:
acceptance over dtypes, batch sizes, vocabularies, input recipes and (T, top_k, top_p) settings, the
Philox uniform bit for bit, greedy and non-finite rows, frequencies, run-to-run bits, untouched neighbours,
the generation state, and the binding's refusals."""
import pytest
import torch

from pyrecover_amd import inference as inf

from tests import sampling_oracles as O

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)
BATCHES = (1, 3, 16)
TEMPS = (0.05, 0.7, 1.0, 1.3, 100.0)
TOP_PS = (1.0, 0.95, 0.5, 1e-6)
WS_WORDS = 65536  # per row


def top_ks(V):
    return (0, 1, 50, V, V + 5)


def _settings(V):
    """Every (T, top_k) pair; top_p runs through its values along the pairs. At V = 7 and 257 the whole product."""
    out = []
    for a, T in enumerate(TEMPS):
        for b, k in enumerate(top_ks(V)):
            out += [(T, k, p) for p in TOP_PS] if V in (7, 257) else [(T, k, TOP_PS[(a + b) % len(TOP_PS)])]
    return out


def _sample(C, x, pos, T, k, p, seed, **kw):
    tok = torch.full((x.shape[0],), -7, dtype=torch.long, device=x.device)
    C.sample_(x, tok, T, k, p, seed, pos=pos, **kw)
    return tok


@pytest.fixture(scope="module")
def C(cuda):
    from pyrecover_amd import _ext

    return _ext.native()


@pytest.mark.parametrize("V", O.VOCABS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_kernel_tokens_are_accepted(cuda, C, dtype, V):
    bad = []
    for ki, kind in enumerate(O.KINDS):
        B = BATCHES[(O.VOCABS.index(V) + ki + DTYPES.index(dtype)) % 3]
        host = O.make_logits(kind, B, V, dtype, 7919 * ki + V + DTYPES.index(dtype))
        if ki % 2:  # ld > V, rows at odd element offsets, padding that would win every draw if it were read
            full = torch.full((B, V + 3), float("inf"), dtype=dtype, device=cuda)
            full[:, V + 1] = float("nan")
            full[:, :V] = host.to(cuda)
            x = full[:, :V]
        else:
            x = host.to(cuda)
        rk = O.Ranking(x, device=cuda)
        ws = torch.empty(B * WS_WORDS, dtype=torch.int32, device=cuda)
        for n, (T, k, p) in enumerate(_settings(V)):
            pos_h = torch.arange(B) * 37 + n
            pos = pos_h.to(cuda, torch.int32)
            u_out = torch.full((B,), -1.0, device=cuda)
            tok = _sample(C, x, pos, T, k, p, 1234, ws=ws, u_out=u_out)
            u = O.uniform(pos_h, 1234)
            assert torch.equal(u_out.double().cpu(), u), (kind, T, k, p)  # bit-equal: u is exact in fp32
            ok = rk.accepted(tok, u, T, k, p)
            if not bool(ok.all()):
                bad += [(kind, B, T, k, p, b, int(tok[b])) for b in range(B) if not ok[b]]
        if ki % 2:
            assert torch.isinf(full[:, V]).all() and torch.isnan(full[:, V + 1]).all()
    assert not bad, bad[:20]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_greedy_is_bit_equal_to_greedy_token(cuda, C, dtype):
    g = torch.Generator().manual_seed(3)
    for V in (1, 7, 300, 2051, 128256):
        x = torch.randn(6, V, generator=g).to(dtype)
        if V >= 300:
            x[1, [250, 17, 99]] = x[1].max() + 1  # ties: the lowest id wins
            x[2] = 0.25
            x[3, 5:] = float("-inf")
            x[4] = float("-inf")
            x[5] = -1.0
            x[5, 7], x[5, 9] = -0.0, 0.0  # one value
        x = x.to(cuda)
        want = inf.greedy_token(x)
        tok = torch.full((6,), -7, dtype=torch.long, device=cuda)
        C.sample_(x, tok, 0.0, 0, 1.0, 0)  # no pos, no workspace: greedy needs neither
        assert torch.equal(tok, want), V
        assert torch.equal(inf.sample_philox(x, torch.zeros(6, device=cuda), 0.0), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_nonfinite_rows_follow_the_total_order(cuda, C, dtype):
    x, want = O.nonfinite_rows(dtype)
    x = x.to(cuda)
    pos = torch.arange(6, device=cuda, dtype=torch.int32)
    for T, k, p in ((0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 5, 0.9)):
        assert _sample(C, x, pos, T, k, p, 1).tolist() == want, (T, k, p)


def test_top_k_one_with_a_unique_maximum_is_greedy_for_every_u(cuda, C):
    x = O.make_logits("peaked", 64, 500, torch.bfloat16, 5).to(cuda)
    want = inf.greedy_token(x)
    for seed in range(4):
        pos = (torch.arange(64) * 3).to(cuda, torch.int32)
        assert torch.equal(_sample(C, x, pos, 1.3, 1, 1.0, seed), want)


def test_frequencies_follow_the_distribution(cuda, C):
    tok, rk, u = O.frequency_case(
        lambda x, pos, seed: _sample(C, x.to(cuda), pos.to(cuda, torch.int32), 1.0, 0, 1.0, seed))
    O.check_frequencies(tok, rk, u)


def test_two_calls_are_bit_identical_and_neighbours_untouched(cuda, C):
    B, V, G = 16, 32000, 64
    x = O.make_logits("normal", B, V, torch.bfloat16, 11).to(cuda)
    x[3] = 0.5  # an all-equal row: every lane of pass 1 hits one bin
    pos = torch.arange(B, device=cuda, dtype=torch.int32) + 5
    tok_buf = torch.full((B + 2 * G,), -7, dtype=torch.long, device=cuda)
    ws_buf = torch.full((B * WS_WORDS + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    u_buf = torch.full((B + 2 * G,), -1.0, device=cuda)
    runs = []
    for _ in range(2):
        for T, k, p in ((0.7, 0, 1.0), (1.0, 50, 0.95), (1.3, 0, 0.5)):
            C.sample_(x, tok_buf[G:G + B], T, k, p, 99, pos=pos, ws=ws_buf[G:G + B * WS_WORDS], u_out=u_buf[G:G + B])
            runs.append(tok_buf[G:G + B].clone())
    assert all(torch.equal(a, b) for a, b in zip(runs[:3], runs[3:]))
    assert not torch.equal(runs[0], runs[1])
    for buf, fill in ((tok_buf, -7), (ws_buf, 0x5A5A5A5A), (u_buf, -1.0)):
        assert (buf[:G] == fill).all() and (buf[-G:] == fill).all()
    assert ((tok_buf[G:G + B] >= 0) & (tok_buf[G:G + B] < V)).all()


def test_generation_state(cuda, C):
    """Rows: 0 live; 1 already done; 2 emits eos; 3 fills its room; 4 one short of its room."""
    B, V, M, G = 5, 300, 6, 8
    x = O.make_logits("peaked", B, V, torch.float16, 21).to(cuda)
    top = inf.greedy_token(x)
    eos = int(top[2])
    assert eos not in (int(top[0]), int(top[3]), int(top[4]))
    out_buf = torch.full((B + 2, M), -1, dtype=torch.long, device=cuda)
    out = out_buf[1:B + 1]
    st_buf = torch.full((3, B + 2 * G), 77, dtype=torch.int32, device=cuda)
    count, room, plen = (st_buf[i, G:G + B] for i in range(3))
    count.copy_(torch.tensor([0, 3, 1, 2, 2]))
    room.copy_(torch.tensor([5, 5, 5, 2, 3]))
    plen.copy_(torch.tensor([4, 9, 2, 7, 1]))
    done_buf = torch.full((B + 2 * G,), 9, dtype=torch.uint8, device=cuda)
    done = done_buf[G:G + B]
    done.copy_(torch.tensor([0, 1, 0, 0, 0], dtype=torch.uint8))
    tok = torch.full((B,), -7, dtype=torch.long, device=cuda)
    state = dict(done=done, count=count, room=room, out=out, eos_id=eos, prompt_len=plen)
    C.sample_(x, tok, 0.0, 0, 1.0, 0, **state)  # greedy: the tokens are known
    t = top.tolist()
    assert tok.tolist() == [t[0], 0, 0, 0, t[4]]  # finished rows feed 0 to the next decode step
    assert done.tolist() == [0, 1, 1, 1, 0] and count.tolist() == [1, 3, 2, 3, 3]
    want = torch.full((B, M), -1, dtype=torch.long)
    want[0, 0], want[2, 1], want[3, 2], want[4, 2] = t[0], eos, t[3], t[4]
    assert torch.equal(out.cpu(), want)  # the done row wrote nothing
    assert (out_buf[0] == -1).all() and (out_buf[-1] == -1).all()
    assert (st_buf[:, :G] == 77).all() and (st_buf[:, -G:] == 77).all() and room.tolist() == [5, 5, 5, 2, 3]
    assert (done_buf[:G] == 9).all() and (done_buf[-G:] == 9).all()
    # a draw: the position is prompt_len + count, read on the device
    u_out = torch.full((B,), -1.0, device=cuda)
    before = count.clone()
    C.sample_(x, tok, 0.9, 0, 1.0, 5, u_out=u_out, **state)
    u = O.uniform((plen + before).cpu(), 5)
    live = torch.tensor([True, False, False, False, True])
    assert torch.equal(u_out.double().cpu()[live], u[live]) and (u_out.cpu()[~live] == -1.0).all()
    assert count.tolist() == [2, 3, 2, 3, 4] and done.tolist() == [0, 1, 1, 1, 1]  # row 4: count 4 > room 3
    assert O.Ranking(x[[0, 4]]).accepted(torch.stack([out[0, 1], out[4, 3]]).cpu(), u[live], 0.9).all()
    # count at max_new: nothing is written, the row finishes
    count.fill_(M)
    done.zero_()
    snap = out.clone()
    C.sample_(x, tok, 0.0, 0, 1.0, 0, **state)
    assert torch.equal(out, snap) and done.tolist() == [1] * B and count.tolist() == [M] * B and tok.tolist() == [0] * B


def test_binding_rejects_bad_arguments(cuda, C):
    x = torch.randn(2, 50, device=cuda).bfloat16()
    tok = torch.zeros(2, dtype=torch.long, device=cuda)
    pos = torch.zeros(2, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        C.sample_(x.float(), tok, 1.0, 0, 1.0, 0, pos=pos)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.sample_(x.cpu(), tok, 1.0, 0, 1.0, 0, pos=pos)
    with pytest.raises(RuntimeError, match="pos"):
        C.sample_(x, tok, 1.0, 0, 1.0, 0, pos=pos.long())
    with pytest.raises(RuntimeError, match="pos"):
        C.sample_(x, tok, 1.0, 0, 1.0, 0)
    with pytest.raises(RuntimeError, match="pos"):
        C.sample_(x, tok, 1.0, 0, 1.0, 0, pos=pos.cpu())
    for p in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(RuntimeError, match="top_p"):
            C.sample_(x, tok, 1.0, 0, p, 0, pos=pos)
    for T in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="temperature"):
            C.sample_(x, tok, T, 0, 1.0, 0, pos=pos)
    with pytest.raises(RuntimeError, match="top_k"):
        C.sample_(x, tok, 1.0, -1, 1.0, 0, pos=pos)
    with pytest.raises(RuntimeError, match="tok"):
        C.sample_(x, tok.int(), 1.0, 0, 1.0, 0, pos=pos)
    with pytest.raises(RuntimeError, match="tok"):
        C.sample_(x, tok[:1], 1.0, 0, 1.0, 0, pos=pos)
    with pytest.raises(RuntimeError, match="ws"):
        C.sample_(x, tok, 1.0, 0, 1.0, 0, pos=pos, ws=torch.zeros(100, dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError, match="stride"):
        C.sample_(x.t().contiguous().t(), tok, 1.0, 0, 1.0, 0, pos=pos)
    with pytest.raises(RuntimeError, match="together"):
        C.sample_(x, tok, 0.0, 0, 1.0, 0, done=torch.zeros(2, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        inf.sample_philox(x, pos, temperature=-1.0)
    t32 = inf.sample_philox(x.float(), pos, 0.8, seed=3)  # fp32 logits take the torch rule, on the GPU too
    assert O.Ranking(x.float()).accepted(t32, O.uniform(pos.cpu(), 3), 0.8).all()
