"""Long and weighted prompts on the CPU: text.parse_prompt_attention and text.ClipTextEncoder(max_prompt_chunks=,
prompt_weighting=) against the restatement in tests/prompt_cpu.py, on tiny random CLIP encoders with a
whitespace tokenizer.  Batched-vs-alone comparisons use 1e-5: fp32 encoders of width 32 with O(1) activations, where a GEMM
that blocks a batch of six rows differently from a batch of one differs by a few fp32 roundings (6e-8) per accumulation."""
import random
import warnings
from types import SimpleNamespace

import pytest
import torch

from tests import prompt_cpu

BOS, EOS, VOCAB = 98, 99, 100
TOL = 1e-5


class StubTokenizer:
    """whitespace -> ids in [1, 97]; ``split`` > 0 cuts words longer than that in two tokens (a tokenizer that counts differently)."""
    model_max_length = 77
    bos_token_id, eos_token_id = BOS, EOS

    def __init__(self, pad_token_id=EOS, split=0):
        self.pad_token_id, self.split = pad_token_id, split

    def _ids(self, text):
        out = []
        for word in text.split():
            parts = [word[:self.split], word[self.split:]] if self.split and len(word) > self.split else [word]
            out += [1 + sum((i + 1) * b for i, b in enumerate(p.encode())) % 97 for p in parts]
        return out

    def __call__(self, text, padding=None, max_length=None, truncation=False, return_tensors=None, add_special_tokens=True):
        if not add_special_tokens:
            assert isinstance(text, str)
            return SimpleNamespace(input_ids=self._ids(text))
        assert padding == "max_length" and truncation and return_tensors == "pt"
        rows = []
        for t in ([text] if isinstance(text, str) else text):
            ids = self._ids(t)[:max_length - 2]
            rows.append([BOS] + ids + [EOS] + [self.pad_token_id] * (max_length - 2 - len(ids)))
        return SimpleNamespace(input_ids=torch.tensor(rows))


def _config():
    from transformers import CLIPTextConfig
    return CLIPTextConfig(vocab_size=VOCAB, hidden_size=32, intermediate_size=64, num_hidden_layers=3, num_attention_heads=4,
                          max_position_embeddings=77, projection_dim=16, bos_token_id=BOS, eos_token_id=EOS, pad_token_id=EOS)


@pytest.fixture(scope="module")
def clip():
    from transformers import CLIPTextModel, CLIPTextModelWithProjection
    torch.manual_seed(0)
    a = CLIPTextModel(_config()).eval()
    b = CLIPTextModelWithProjection(_config()).eval()
    return a, b


def _encoder(clip, xl=False, split=0, **kw):
    from elasticdiffusion_official_amd.text import ClipTextEncoder
    toks = [StubTokenizer()] + ([StubTokenizer(pad_token_id=0, split=split)] if xl else [])
    return ClipTextEncoder(toks, list(clip[:2 if xl else 1]), xl, "cpu", **kw)


def _words(n, seed=0):
    rnd = random.Random(seed)
    return " ".join("".join(rnd.choice("abcdefghij") for _ in range(rnd.randint(2, 4))) for _ in range(n))


# ---- the parser ------------------------------------------------------------------------------------------------------
WORKED = [
    ("a (((house:1.3)) [on] a (hill:0.5), sun, (((sky))).",
     [("a ", 1.0), ("house", 1.3 * 1.1 * 1.1), (" ", 1.1), ("on", 1.0), (" a ", 1.1), ("hill", 0.55), (", sun, ", 1.1),
      ("sky", 1.1 ** 4), (".", 1.1)]),
    ("(unbalanced", [("unbalanced", 1.1)]),
    ("\\(literal\\]", [("(literal]", 1.0)]),
    ("(a)(b)", [("ab", 1.1)]),
    ("plain text: no syntax", [("plain text: no syntax", 1.0)]),
    ("", [("", 1.0)]),
]


@pytest.mark.parametrize("parse", ["product", "restatement"])
@pytest.mark.parametrize("text,want", WORKED)
def test_parser_worked_examples(parse, text, want):
    from elasticdiffusion_official_amd.text import parse_prompt_attention
    got = (parse_prompt_attention if parse == "product" else prompt_cpu.parse_weights)(text)
    assert [g[0] for g in got] == [w[0] for w in want], got
    assert [g[1] for g in got] == pytest.approx([w[1] for w in want], rel=1e-12), got


def test_parser_against_the_restatement_on_random_bracket_strings():
    from elasticdiffusion_official_amd.text import parse_prompt_attention
    rnd = random.Random(20)
    atoms = ["(", ")", "[", "]", "\\(", "\\)", "\\[", "\\]", "\\\\", "\\", ":", ":1.3)", ": 0.5 )", ":.25)", ":2.)", ":1.2.3)", ":x)",
             ":-1)", "cat", " ", "a b", ",", "7", ".", ":+1.5)"]
    for _ in range(3000):
        s = "".join(rnd.choice(atoms) for _ in range(rnd.randint(0, 12)))
        got, want = parse_prompt_attention(s), prompt_cpu.parse_weights(s)
        assert [g[0] for g in got] == [w[0] for w in want], (s, got, want)
        assert [g[1] for g in got] == pytest.approx([w[1] for w in want], rel=1e-12), (s, got, want)


# ---- defaults --------------------------------------------------------------------------------------------------------
def _today(clip, xl, prompts, split=0):
    """What ClipTextEncoder.__call__ computed before the two keywords existed."""
    toks = [StubTokenizer()] + ([StubTokenizer(pad_token_id=0, split=split)] if xl else [])
    outs = []
    with torch.no_grad():
        for tok, enc in zip(toks, clip):
            ids = tok(prompts, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
            outs.append(enc(ids.input_ids, output_hidden_states=True))
    if xl:
        return torch.cat([outs[0].hidden_states[-2], outs[1].hidden_states[-2]], dim=-1), outs[1][0]
    return outs[0][0], outs[0][0]


@pytest.mark.parametrize("xl", [False, True])
def test_defaults_are_todays_output_and_a_short_prompt_is_unchanged_by_the_keywords(clip, xl):
    prompts = [_words(12, 1), _words(75, 2), _words(90, 3) + " (x:1.3)"]      # the last one is truncated by default
    e0, p0 = _today(clip, xl, prompts)
    enc = _encoder(clip, xl)
    assert enc.chunks(prompts) == 1
    e, p = enc(prompts)
    assert torch.equal(e, e0) and torch.equal(p, p0) and e.shape[1] == 77
    e, p = enc(prompts, min_chunks=1)
    assert torch.equal(e, e0) and torch.equal(p, p0)
    short = prompts[:2]                                                     # <= 75 tokens: no second chunk, no weights
    e0, p0 = _today(clip, xl, short)
    e, p = _encoder(clip, xl, max_prompt_chunks=3, prompt_weighting=True)(short)
    assert torch.equal(e, e0) and torch.equal(p, p0)


# ---- chunks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tokens,n_chunks", [(75, 1), (76, 2), (150, 2), (151, 3)])
def test_chunk_counts(clip, n_tokens, n_chunks):
    enc = _encoder(clip, max_prompt_chunks=3)
    prompt = _words(n_tokens, n_tokens)
    assert enc.chunks(prompt) == n_chunks == enc.chunks(["short", prompt])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        e, _ = enc(prompt)
    assert e.shape == (1, 77 * n_chunks, 32)


@pytest.mark.parametrize("xl", [False, True])
def test_every_chunk_is_the_encoder_on_that_chunks_row_alone(clip, xl):
    prompts = [_words(160, 4), _words(20, 5), _words(76, 6)]
    enc = _encoder(clip, xl, max_prompt_chunks=3)
    e, p = enc(prompts)
    want, pooled, n, dropped = prompt_cpu.encode(enc.tokenizers, enc.encoders, xl, prompts, max_chunks=3)
    assert n == 3 and dropped == 0 and e.shape == want.shape == (3, 231, 64 if xl else 32)
    assert float((e - want).abs().max()) < TOL
    assert float((p - pooled).abs().max()) < TOL
    # chunk 0 of the short prompt is what the default call gives for it; its other chunks are the empty chunk's encoding
    e1, _ = _encoder(clip, xl)(prompts[1])
    assert float((e[1, :77] - e1[0]).abs().max()) < TOL
    empty, _ = _encoder(clip, xl)("")
    assert float((e[1, 77:154] - empty[0]).abs().max()) < TOL and float((e[1, 154:] - empty[0]).abs().max()) < TOL


def test_min_chunks_pads_with_the_empty_chunks_encoding(clip):
    enc = _encoder(clip, max_prompt_chunks=3)
    prompt = _words(30, 7)
    e1, _ = enc(prompt)
    e3, _ = enc(prompt, min_chunks=3)
    empty, _ = enc("")
    assert e1.shape[1] == 77 and e3.shape[1] == 231
    assert float((e3[0, :77] - e1[0]).abs().max()) < TOL
    for c in (1, 2):
        assert float((e3[0, 77 * c:77 * (c + 1)] - empty[0]).abs().max()) < TOL
    # the default encoder pads too when asked to (a job of a fused batch whose neighbour has a long prompt)
    e2, _ = _encoder(clip)(prompt, min_chunks=2)
    assert e2.shape[1] == 154 and float((e2[0] - e3[0, :154]).abs().max()) < TOL


def test_truncation_at_the_cap_warns_once_with_the_count(clip):
    enc = _encoder(clip, max_prompt_chunks=2)
    prompt = _words(163, 8)
    assert enc.chunks(prompt) == 2
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        e, _ = enc(prompt)
    assert len(rec) == 1 and "13 tokens dropped" in str(rec[0].message), [str(r.message) for r in rec]
    want, _, n, dropped = prompt_cpu.encode(enc.tokenizers, enc.encoders, False, prompt, max_chunks=2)
    assert n == 2 and dropped == 13
    kept, *_ = prompt_cpu.encode(enc.tokenizers, enc.encoders, False, " ".join(prompt.split()[:150]), max_chunks=2)
    assert torch.equal(want, kept)                                        # the first 150 tokens are what is encoded
    assert e.shape == (1, 154, 32) and float((e - want).abs().max()) < TOL


# ---- weights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xl", [False, True])
def test_weights(clip, xl):
    base = _words(100, 9).split()
    plain = " ".join(base)
    weighted = " ".join(base[:10]) + " (" + " ".join(base[10:20]) + ":1.4) [" + " ".join(base[20:90]) + "] " + " ".join(base[90:])
    enc = _encoder(clip, xl, max_prompt_chunks=2, prompt_weighting=True)
    off = _encoder(clip, xl, max_prompt_chunks=2)
    e, p = enc([plain, weighted])
    e_off, p_off = off([plain, plain])
    assert torch.equal(e[0], e_off[0])                                   # all-1 prompt: not touched, bit for bit
    assert torch.equal(p, p_off)                                         # pooled: never weighted
    assert not torch.equal(e[1], e_off[1])
    widths = [32, 32] if xl else [32]
    lo = 0
    for wd in widths:                                                    # the mean is restored per encoder output
        got, was = e[1, :, lo:lo + wd], e_off[1, :, lo:lo + wd]
        assert abs(float(got.mean()) - float(was.mean())) <= 4 * 2 ** -23 * max(abs(float(was.mean())), float(was.abs().mean()))
        lo += wd
    want, pooled, n, _ = prompt_cpu.encode(enc.tokenizers, enc.encoders, xl, [plain, weighted], max_chunks=2, weighting=True)
    assert n == 2 and float((e - want).abs().max()) < TOL and float((p - pooled).abs().max()) < TOL
    if xl:                                                               # pooled: text_encoder_2's projection of the FIRST chunk
        first = " ".join(base[:75])
        assert float((p[0] - _today(clip, True, [first])[1][0]).abs().max()) < TOL
    # the weight scales a token's embedding: token 11 (weight 1.4) against token 1 (weight 1), up to the common mean factor
    ratio = (e[1, 11, :32] / e_off[1, 11, :32]) / (e[1, 1, :32] / e_off[1, 1, :32])
    assert float((ratio - 1.4).abs().max()) < 1e-3


def test_weight_syntax_is_literal_text_without_prompt_weighting(clip):
    e, _ = _encoder(clip, max_prompt_chunks=2)("a (cat:1.3)")
    e0, _ = _today(clip, False, ["a (cat:1.3)"])
    assert torch.equal(e, e0)


def test_sdxl_tokenizers_that_disagree_are_both_padded_to_the_larger_count(clip):
    prompt = " ".join(["abcdefgh"] * 40)                                 # 40 tokens for tokenizer 1, 80 for tokenizer 2
    enc = _encoder(clip, True, split=4, max_prompt_chunks=3)
    assert enc.chunks(prompt) == 2
    e, p = enc(prompt)
    assert e.shape == (1, 154, 64)
    want, pooled, n, _ = prompt_cpu.encode(enc.tokenizers, enc.encoders, True, prompt, max_chunks=3)
    assert n == 2 and float((e - want).abs().max()) < TOL and float((p - pooled).abs().max()) < TOL
    empty = clip[0](torch.tensor([[BOS, EOS] + [EOS] * 75]), output_hidden_states=True).hidden_states[-2][0].detach()
    assert float((e[0, 77:, :32] - empty).abs().max()) < TOL              # encoder 1's second chunk is the empty one


# ---- pipeline plumbing that needs no GPU -----------------------------------------------------------------------------
def test_graph_key_separates_text_lengths_and_keeps_the_77_token_key_stable():
    from elasticdiffusion_official_amd.graphs import GraphedForward
    t77, t154 = torch.empty(20, 77, 8), torch.empty(20, 154, 8)
    pooled = torch.empty(20, 4)
    k = GraphedForward._key
    assert k((20, 4, 8, 8), torch.float16, None, (), False, t77, pooled) != k((20, 4, 8, 8), torch.float16, None, (), False, t154, pooled)
    assert k((20, 4, 8, 8), torch.float16, None, (), False, t77, pooled) == k((20, 4, 8, 8), torch.float16, None, text=t77.clone(), pooled=pooled)
    assert k((20, 4, 8, 8), torch.float16, None, (), False, t77, None) != k((20, 4, 8, 8), torch.float16, None, (), False, t77, pooled)


def test_command_line_flags_parse():
    from elasticdiffusion_official_amd.__main__ import build_parser
    opt = build_parser().parse_args([])
    assert opt.max_prompt_chunks == 1 and opt.prompt_weighting is False
    opt = build_parser().parse_args(["--max_prompt_chunks", "3", "--prompt_weighting", "true"])
    assert opt.max_prompt_chunks == 3 and opt.prompt_weighting is True


def test_flash_dispatch_for_long_prompts():
    """Two chunks (154 keys) stream at Nq >= 4096; three chunks keep the pipelined kernel, and everything
    test_flash_variant_heuristic pins stays."""
    from elasticdiffusion_official_amd import ops
    pipe = ops.FLASH_DEFAULT_PIPE
    assert ops._flash_variant(20, 10, 4096, 154) == 8 and ops._flash_variant(40, 10, 4096, 128) == 8
    assert ops._flash_variant(20, 10, 4096, 160) == 8 and ops._flash_variant(20, 10, 4096, 161) == pipe
    assert ops._flash_variant(20, 20, 1024, 154) == pipe
    assert ops._flash_variant(20, 10, 4096, 231) == pipe and ops._flash_variant(20, 20, 1024, 231) == pipe
    assert ops._flash_variant(20, 10, 4096, 77) == 8 and ops._flash_variant(1, 10, 4096, 100) == 0
    assert ops._flash_variant(20, 10, 4096, 127) == 0 and ops._flash_variant(20, 10, 4096, 4096) == pipe
