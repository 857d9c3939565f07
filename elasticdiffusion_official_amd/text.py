"""CLIP text encoding for the pipeline's ``text_encoder=`` hook (elastic_diffusion.py:248-265).

The reference tokenises with ``CLIPTokenizer`` (padding to ``model_max_length``, truncation) and runs
``CLIPTextModel`` (+ ``CLIPTextModelWithProjection`` for SDXL) from ``transformers``:
  * SD 1.x / 2.x : embeddings = encoder(...)[0] (last hidden state), "pooled" = the same tensor      (ED:260-262)
  * SDXL         : embeddings = concat(hidden_states[-2] of both encoders, dim=-1),
                   pooled = text_encoder_2(...)[0] (the projected text embedding)                   (ED:256-259)
No CLIP weights or vocab files exist in the build image, so the pipeline defaults to synthetic embeddings; with a
local HF snapshot ``load_clip(model_dir, xl)`` builds the real thing.

Two opt-in extensions the reference does not have (tests/prompt_cpu.py restates them):
  * ``max_prompt_chunks`` > 1: a prompt longer than 75 tokens is encoded in 75-token chunks, concatenated on the token axis
    ([B, 77 n, D]) instead of being truncated;
  * ``prompt_weighting``: ``(x)``, ``[x]``, ``(x:1.3)`` scale the embeddings of the tokens of ``x``.
"""
import os
import re
import warnings

import torch

CHUNK_TOKENS = 75   # prompt tokens per chunk; with bos and eos a chunk is the 77 positions CLIP was trained on

_ATTENTION = re.compile(r"\\[()\[\]\\]|\(|\[|:\s*([+-]?(?:\d+\.?\d*|\.\d+))\s*\)|\)|\]|[^\\()\[\]:]+|:|\\")


def parse_prompt_attention(text):
    """``'a (b:1.3) [c]'`` -> ``[["a ", 1.0], ["b", 1.3], [" ", 1.0], ["c", 1 / 1.1]]``: the weight syntax of the A1111 web UI.
    ``(x)`` multiplies by 1.1, ``[x]`` by 1 / 1.1, ``(x:w)`` by w (a ``:w`` counts only directly before the closing round bracket),
    nesting multiplies, a backslash makes a bracket or a backslash literal, brackets still open at the end of the string apply
    from where they opened, a closing bracket without an opening one is text.  Adjacent fragments of equal weight are merged;
    an empty result is ``[["", 1.0]]``."""
    res, rounds, squares = [], [], []

    def scale(start, factor):
        for frag in res[start:]:
            frag[1] *= factor

    for m in _ATTENTION.finditer(text):
        tok, w = m.group(0), m.group(1)
        if len(tok) == 2 and tok[0] == "\\":
            res.append([tok[1], 1.0])
        elif tok == "(":
            rounds.append(len(res))
        elif tok == "[":
            squares.append(len(res))
        elif w is not None and rounds:
            scale(rounds.pop(), float(w))
        elif tok == ")" and rounds:
            scale(rounds.pop(), 1.1)
        elif tok == "]" and squares:
            scale(squares.pop(), 1 / 1.1)
        else:
            res.append([tok, 1.0])
    for start in rounds:
        scale(start, 1.1)
    for start in squares:
        scale(start, 1 / 1.1)
    merged = []
    for frag, w in res:
        if merged and merged[-1][1] == w:
            merged[-1][0] += frag
        else:
            merged.append([frag, w])
    return merged or [["", 1.0]]


class ClipTextEncoder:
    """Callable ``prompts -> (text_embeddings, pooled)`` over already constructed tokenizers / encoders.

    ``max_prompt_chunks`` (default 1) and ``prompt_weighting`` (default False) are opt-in; with the defaults a call runs the
    reference's tokenizer call and nothing else.  Otherwise every prompt becomes a stream of (token id, weight): each weighted
    fragment is tokenised on its own without special tokens (a prompt without syntax is one fragment), the stream is cut
    every 75 tokens, and chunk c is ``[bos] + ids + [eos] + [pad] * (75 - len)`` with weight 1 on bos / eos / pad.  All chunks
    of all prompts go through the encoder as one [B n, 77] batch and come back as [B, 77 n, D]."""

    def __init__(self, tokenizers, encoders, xl, device="cpu", max_prompt_chunks=1, prompt_weighting=False):
        assert len(tokenizers) == len(encoders) == (2 if xl else 1)
        if int(max_prompt_chunks) < 1:
            raise ValueError(f"max_prompt_chunks must be >= 1, got {max_prompt_chunks}")
        self.tokenizers, self.encoders, self.xl, self.device = tokenizers, encoders, xl, device
        self.max_prompt_chunks, self.prompt_weighting = int(max_prompt_chunks), bool(prompt_weighting)

    def _encode(self, prompts, k):
        tok = self.tokenizers[k]
        ids = tok(prompts, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
        return self.encoders[k](ids.input_ids.to(self.device), output_hidden_states=True)

    # ---- long / weighted prompts -------------------------------------------------------------------------------------
    @property
    def _plain(self):
        return self.max_prompt_chunks == 1 and not self.prompt_weighting

    def _stream(self, prompt, k):
        """-> (ids, weights) of one prompt for tokenizer k, before any cut."""
        tok = self.tokenizers[k]
        ids, weights = [], []
        for frag, w in (parse_prompt_attention(prompt) if self.prompt_weighting else [[prompt, 1.0]]):
            t = list(tok(frag, add_special_tokens=False).input_ids)
            ids += t
            weights += [w] * len(t)
        return ids, weights

    def _streams(self, prompts):
        """-> (streams[k][b] = (ids, weights) cut at the cap, chunk count over prompts and tokenizers, tokens dropped)."""
        cap = CHUNK_TOKENS * self.max_prompt_chunks
        streams, n = [], 1
        lost = [0] * len(prompts)
        for k in range(len(self.tokenizers)):
            row = []
            for b, prompt in enumerate(prompts):
                ids, weights = self._stream(prompt, k)
                lost[b] = max(lost[b], len(ids) - cap)
                ids, weights = ids[:cap], weights[:cap]
                n = max(n, -(-len(ids) // CHUNK_TOKENS))
                row.append((ids, weights))
            streams.append(row)
        dropped = sum(v for v in lost if v > 0)
        return streams, n, dropped

    def chunks(self, prompts):
        """Number of 77-position chunks a call with these prompts produces (the maximum over the prompts and, for SDXL, over
        both tokenizers; at most ``max_prompt_chunks``), without encoding anything."""
        if isinstance(prompts, str):
            prompts = [prompts]
        return 1 if self._plain else self._streams(prompts)[1]

    def _rows(self, stream, n, k):
        """-> (ids [n, 77] long, weights [77 n] float32) of one prompt's stream padded to n chunks."""
        tok = self.tokenizers[k]
        ids, weights = stream
        id_rows, w_rows = [], []
        for c in range(n):
            part = ids[CHUNK_TOKENS * c: CHUNK_TOKENS * (c + 1)]
            fill = CHUNK_TOKENS - len(part)
            id_rows.append([tok.bos_token_id] + part + [tok.eos_token_id] + [tok.pad_token_id] * fill)
            w_rows += [1.0] + weights[CHUNK_TOKENS * c: CHUNK_TOKENS * (c + 1)] + [1.0] * (1 + fill)
        return torch.tensor(id_rows, dtype=torch.long), torch.tensor(w_rows, dtype=torch.float32)

    def _encode_chunks(self, streams, n, k):
        """-> (encoder output of the [B n, 77] chunk batch, weights [B, 77 n])."""
        rows = [self._rows(s, n, k) for s in streams[k]]
        ids = torch.cat([r[0] for r in rows])
        return self.encoders[k](ids.to(self.device), output_hidden_states=True), torch.stack([r[1] for r in rows])

    @staticmethod
    def _weighted(z, w):
        """z [B, 77 n, D] with the token weights w [B, 77 n] applied per prompt, each prompt's mean restored; a prompt whose
        weights are all 1 keeps its bits."""
        touched = [b for b in range(z.shape[0]) if bool((w[b] != 1).any())]
        if not touched:
            return z
        z = z.clone()
        for b in touched:
            m0 = z[b].mean()
            zb = z[b] * w[b].to(device=z.device, dtype=z.dtype)[:, None]
            z[b] = zb * (m0 / zb.mean())
        return z

    @torch.no_grad()
    def __call__(self, prompts, min_chunks=None):
        """``min_chunks``: produce at least this many chunks (missing ones are empty: bos, eos, 75 pads), so that prompt and
        negative prompt -- or the jobs of one fused batch -- end with the same token count."""
        if isinstance(prompts, str):
            prompts = [prompts]
        if self._plain and (min_chunks is None or int(min_chunks) <= 1):
            if self.xl:
                a, b = self._encode(prompts, 0), self._encode(prompts, 1)
                return torch.cat([a.hidden_states[-2], b.hidden_states[-2]], dim=-1), b[0]
            e = self._encode(prompts, 0)[0]
            return e, e
        streams, n, dropped = self._streams(prompts)
        if dropped:
            warnings.warn(f"prompt longer than max_prompt_chunks={self.max_prompt_chunks} x {CHUNK_TOKENS} tokens: "
                          f"{dropped} tokens dropped")
        if min_chunks is not None:
            n = max(n, int(min_chunks))
        B = len(prompts)
        if self.xl:
            (a, wa), (b, wb) = self._encode_chunks(streams, n, 0), self._encode_chunks(streams, n, 1)
            za = self._weighted(a.hidden_states[-2].reshape(B, 77 * n, -1), wa)
            zb = self._weighted(b.hidden_states[-2].reshape(B, 77 * n, -1), wb)
            pooled = b[0]
            return torch.cat([za, zb], dim=-1), pooled.reshape(B, n, -1)[:, 0].contiguous()   # pooled: first chunk, never weighted
        out, w = self._encode_chunks(streams, n, 0)
        e = out[0].reshape(B, 77 * n, -1)
        z = self._weighted(e, w)
        return z, e    # "pooled" (unused by the SD 1.x / 2.x UNet) is the unweighted tensor: the same object when no weight applies


def load_clip(model_dir, xl, device="cuda", dtype=torch.float32, max_prompt_chunks=1, prompt_weighting=False):
    """HF snapshot layout: tokenizer/, text_encoder/ (+ tokenizer_2/, text_encoder_2/ for SDXL)  (ED:145-151)."""
    from transformers import CLIPTextModel, CLIPTextModelWithProjection, CLIPTokenizer
    toks = [CLIPTokenizer.from_pretrained(os.path.join(model_dir, "tokenizer"))]
    encs = [CLIPTextModel.from_pretrained(os.path.join(model_dir, "text_encoder"), torch_dtype=dtype).to(device).eval()]
    if xl:
        toks.append(CLIPTokenizer.from_pretrained(os.path.join(model_dir, "tokenizer_2")))
        encs.append(CLIPTextModelWithProjection.from_pretrained(os.path.join(model_dir, "text_encoder_2"),
                                                                torch_dtype=dtype).to(device).eval())
    return ClipTextEncoder(toks, encs, xl, device, max_prompt_chunks, prompt_weighting)
