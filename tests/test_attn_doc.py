"""Document-masked attention away from the GPU: the tables, the fp32 torch path, the refusals, the programs' param."""
import pytest
import torch

EOS, S = 7, 12
ROWS = [[1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6],      # no EOS
        [7, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6],      # EOS at position 0
        [1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 7],      # EOS at position S - 1
        [1, 2, 3, 7, 7, 6, 1, 2, 7, 4, 5, 6]]      # two adjacent EOS, and a third


def _tables(row):
    """start / end of one row by the definition: t opens a document iff t == 0 or row[t - 1] is the EOS"""
    opens = [t for t in range(len(row)) if t == 0 or row[t - 1] == EOS] + [len(row)]
    return [max(o for o in opens if o <= t) for t in range(len(row))], [min(o for o in opens if o > t) for t in range(len(row))]


def _state():
    from polyaxon_amd.ops.attn_doc import AttnDocState

    st = AttnDocState("cpu", len(ROWS), S, EOS)
    assert st.start.dtype == st.end.dtype == torch.int32
    assert st.start.tolist() == [[0] * S] * 4 and st.end.tolist() == [[S] * S] * 4   # one document per row
    st.update(torch.tensor(ROWS))                                                    # a batch whose rows differ
    return st, AttnDocState


def test_update_against_a_loop_over_the_tokens():
    st, State = _state()
    assert st.start.tolist() == [_tables(r)[0] for r in ROWS] and st.end.tolist() == [_tables(r)[1] for r in ROWS]
    for bad in (-1, 0.5, True, 2 ** 31):
        with pytest.raises(ValueError):
            State("cpu", 1, S, bad)


def test_fallback_is_attention_on_each_document_and_refusals():
    from polyaxon_amd.ops.attention import flash_attention
    from polyaxon_amd.ops.attn_window import AttnWindowState

    g, (st, State) = torch.Generator().manual_seed(5), _state()
    q, k, v = (torch.randn(len(ROWS), h, S, 16, generator=g, requires_grad=True) for h in (4, 2, 2))
    out = flash_attention(q, k, v, causal=True, scale=0.5, doc=st)
    want = torch.zeros_like(out)
    for b, row in enumerate(ROWS):   # plain causal attention on every document's slice
        for lo, hi in sorted(set(zip(*_tables(row)))):
            want[b, lo:hi] = flash_attention(q[b:b + 1, :, lo:hi], k[b:b + 1, :, lo:hi], v[b:b + 1, :, lo:hi], scale=0.5)
    dout = torch.randn(out.shape, generator=g)
    assert torch.allclose(out, want, atol=1e-6)
    for a, b in zip(torch.autograd.grad(out, (q, k, v), dout), torch.autograd.grad(want, (q, k, v), dout)):
        assert torch.allclose(a, b, atol=1e-5)
    for kw in (dict(causal=False), dict(window=AttnWindowState("cpu", 4)), dict(k=k[:, :, :8], v=v[:, :, :8]),
               dict(doc=State("cpu", len(ROWS), S + 1, EOS)), dict(doc=State("cpu", 1, S, EOS))):
        with pytest.raises(ValueError):
            flash_attention(**{**dict(q=q, k=k, v=v, causal=True, doc=st), **kw})


def test_program_param_and_rejections():
    from polyaxon_amd.polyflow.programs import build_program

    plain = build_program("gpt2_tiny", {}, "cpu")
    prog = build_program("gpt2_tiny", {"attn_doc_eos": 3, "attn_dropout": True}, "cpu")
    assert prog.info["attn_doc_eos"] == 3 and "attn_doc_eos" not in plain.info
    assert prog.hp_keys == plain.hp_keys + ("attn_dropout",)          # part of the program, not a per-trial value
    ex = prog.executor
    assert all(b.attn._doc is ex.attn_doc for b in ex.model.blocks) and ex.attn_doc.eos_id == 3
    for name, params in (("resnet_tiny", {"attn_doc_eos": 3}), ("mlp", {"attn_doc_eos": 3}),
                         ("gpt2_tiny", {"attn_doc_eos": 3, "attn_window": True})):
        with pytest.raises(ValueError, match="attn_doc_eos"):
            build_program(name, params, "cpu")
