"""The one per-row sampler state of a ``DecodeState`` on the GPU (csm/sampling.py, ``RowSampler``), on the tiny model of
tests/test_row_sampling_gpu.py with three rows: a state raised from level 1 to 2 to 3 to 4 at identity extras draws, level by level, the
codes the scalar path draws for each row's pair; the write that raises a level reaches every row, later ones one row; each level
has its graph key and a parameter write replays the same captured graph.  Codes are compared with torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
K, V, B = 32, 2051, 3
PAIRS = [(0.8, 12), (0.6, 1), (1.2, 200)]           # (the one-wave and the block-wide finish among them)
IDENTITY = (1.0, 0.0, 1.0, 64)                      # top_p, min_p, penalty, window: a higher level that changes nothing
RAISE = {1: lambda st, b, t, k: st.set_row_sampling(b, t, k),
         2: lambda st, b, t, k: st.set_row_filters(b, 1.0, 0.0),
         3: lambda st, b, t, k: st.set_row_processors(b, t, k, *IDENTITY),
         4: lambda st, b, t, k: st.set_row_typical(b, t, k, *IDENTITY, 1.0)}
KEYS = {1: (None, None), 2: (None, None, "filters"), 3: (None, None, "processors"), 4: (None, None, "typical")}


@pytest.fixture(scope="module")
def world(dev):
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, V, K), device="cuda", seed=2)
    m.engine._need()
    g = torch.Generator().manual_seed(7)
    toks, msks = [], []
    for b in range(B):
        tk = torch.zeros(4 + b, K + 1, dtype=torch.long)
        tk[:, -1] = torch.randint(3, 200, (4 + b,), generator=g)
        mk = torch.zeros(4 + b, K + 1, dtype=torch.bool)
        mk[:, -1] = True
        toks.append(tk.cuda())
        msks.append(mk.cuda())
    gq = torch.Generator(device="cuda").manual_seed(8)
    noise = [list(torch.empty(K, B, V, dtype=torch.float32, device="cuda").exponential_(1, generator=gq)) for _ in range(4)]
    return dict(m=m, toks=toks, msks=msks, noise=noise)


def _mirror_is_buffers(st):
    s = st.sampler
    for j, buf in enumerate(s.params):
        want = torch.tensor([s.rows[b][j] for b in range(B)], dtype=buf.dtype).t()
        assert buf.shape == (K, B) and buf.is_contiguous() and torch.equal(buf.cpu(), want), j


@torch.no_grad()
def test_a_higher_level_at_identity_is_the_lower_levels_draw(world):
    from csm.engine import DecodeState
    e, noise = world["m"].engine, world["noise"][0]
    st = DecodeState(e, B)
    last_h = st.prefill_ragged(world["toks"], world["msks"])
    scalar = [e._frame_tail(st, last_h, t, k, noise) for t, k in PAIRS]     # [B, K] each: every row with pair b
    want = torch.stack([scalar[b][b] for b in range(B)])
    assert st.sampler.level == 0 and st.graph_key is None and not torch.equal(scalar[0][1], scalar[1][1])
    for level in (1, 2, 3, 4):
        for b, (t, k) in enumerate(PAIRS):
            RAISE[level](st, b, t, k)
        assert st.sampler.level == level
        _mirror_is_buffers(st)
        assert st.sampler.rows == [((t,) * K, (k,) * K) + tuple((v,) * K for v in IDENTITY + (1.0,)) for t, k in PAIRS]
        got = e._frame_tail(st, last_h, None, None, noise)
        assert got.shape == (B, K) and torch.equal(got, want), level
        if level == 3:
            assert st.row_processors is not None and st.sampler.hist_frame.tolist() == [1] * B      # (the level-3 frame was counted)
            assert torch.equal(st.sampler.code_hist[:, :, 0], want)
    assert st.row_typical is not None and st.row_processors is None and st.sampler.hist_frame.tolist() == [2] * B
    assert torch.equal(st.sampler.code_hist[:, :, 1], want)                 # (... and the level-4 frame, in the same rings)


def test_the_write_that_raises_a_level_reaches_every_row(world):
    from csm.engine import DecodeState
    st = DecodeState(world["m"].engine, B)
    st.set_row_sampling(1, 1.25, 7)
    assert st.row_sampling == [(1.25, 7)] * B and st.row_filters is None and st.row_processors is None
    _mirror_is_buffers(st)
    st.set_row_sampling(0, 0.5, 3)
    pairs = [(0.5, 3), (1.25, 7), (1.25, 7)]
    assert st.row_sampling == pairs
    st.set_row_filters(2, 0.5, 0.1)
    assert st.row_filters == [(0.5, 0.1)] * B and st.row_sampling == pairs
    _mirror_is_buffers(st)
    six = ([0.9] + [0.6] * (K - 1), 20, 0.9, 0.05, 1.3, list(range(K)))
    st.set_row_processors(0, *six)
    row0 = (tuple(six[0]), (20,) * K, (0.9,) * K, (0.05,) * K, (1.3,) * K, tuple(range(K)))
    assert st.row_processors == [row0] * B and st.row_sampling is None and st.row_filters is None
    _mirror_is_buffers(st)
    st.set_row_processors(2, 0.7, 20, 0.9, 0.05, 1.3, 16)                   # ... and a later one its own row only
    assert st.row_processors[:2] == [row0] * 2 and st.row_processors[2][0] == (0.7,) * K and st.row_processors[2][5] == (16,) * K
    _mirror_is_buffers(st)
    per = tuple([0.5] + [0.9] * (K - 1))
    st.set_row_typical(1, *six, list(per))                                  # level 4: the seven reach every row ...
    assert st.row_typical == [row0 + (per,)] * B and st.row_processors is None
    _mirror_is_buffers(st)
    st.set_row_typical(0, *six, 0.25)                                       # ... and a later one its own row only
    assert st.row_typical[0] == row0 + ((0.25,) * K,) and st.row_typical[1:] == [row0 + (per,)] * 2
    _mirror_is_buffers(st)


@pytest.mark.parametrize("level", [1, 2, 3, 4])
@torch.no_grad()
def test_each_level_has_its_graph_key_and_a_write_replays_the_same_graph(world, level):
    from csm.engine import DecodeState
    m, noise = world["m"], world["noise"]
    e = m.engine
    amask = torch.cat([torch.ones(B, 1, K, dtype=torch.bool), torch.zeros(B, 1, 1, dtype=torch.bool)], 2).cuda()
    assert getattr(m, "use_hip_graph", True)

    def run(graph):
        st = DecodeState(e, B)
        for lv in range(1, level + 1):
            for b, (t, k) in enumerate(PAIRS):
                RAISE[lv](st, b, t, k)
        out = [e._frame_tail(st, st.prefill_ragged(world["toks"], world["msks"]), None, None, noise[0])]
        captured = None
        for f in (1, 2, 3):                                                 # eager (warm-up), captured, replayed
            cur = torch.cat([out[-1].long(), torch.zeros(B, 1, dtype=torch.long, device="cuda")], 1).unsqueeze(1)
            if graph:
                out.append(st.graph_frame(cur, amask, None, None, noise[f]))
            else:
                st._advance()
                out.append(e._decode_frame(st, cur, amask, None, None, noise[f]))
            if f == 2:
                captured = st.graph
                assert (captured is not None) == graph
                RAISE[1](st, 1, 1.1, 65)                                    # between the replays: the pair, and this level's own
                if level == 2:
                    st.set_row_filters(1, 0.7, 0.01)
                if level == 3:
                    st.set_row_processors(1, 1.1, 65, 0.7, 0.01, 1.5, 2)
                if level == 4:
                    st.set_row_typical(1, 1.1, 65, 0.7, 0.01, 1.5, 2, 0.6)
                _mirror_is_buffers(st)
        assert st.graph is captured and st.sampler.level == level
        if graph:
            assert st.graph_key == KEYS[level] == st.sampler.graph_key(None, None)
        return torch.stack(out, 2)
    graphed, eager = run(True), run(False)
    assert torch.equal(graphed, eager)                                      # (the replay read what was written)
