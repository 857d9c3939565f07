"""Long and weighted prompts, restated in plain Python / torch-CPU ops (test infrastructure).

An independent statement of what ``text.ClipTextEncoder(max_prompt_chunks=, prompt_weighting=)`` computes: a character-level
parser of the weight syntax (no regular expression, unlike the product), the cut of the (token id, weight) stream into
75-token chunks, and the per-prompt weighting with the mean restored.  **Parity unpinned** to the A1111 web UI, diffusers'
``lpw_stable_diffusion(_xl)`` and compel: none of them can be installed here, so the rules below are the specification.
"""
import math

import torch

CHUNK = 75


def parse_weights(text):
    """-> [(fragment, weight)]; the rules of DESIGN.md section 21.1, one character at a time."""
    chars = []            # [char, weight]
    opened = []           # (kind, index into chars where the bracket's content starts)
    i, n = 0, len(text)

    def mul(start, f):
        for c in chars[start:]:
            c[1] *= f

    def last_open(kind):
        for j in range(len(opened) - 1, -1, -1):
            if opened[j][0] == kind:
                return j
        return None

    def weight_suffix(at):
        """``: w )`` starting at text[at] == ':' -> (w, index after ')') or None."""
        j = at + 1
        while j < n and text[j].isspace():
            j += 1
        k = j
        if k < n and text[k] in "+-":
            k += 1
        d0 = k
        while k < n and text[k].isdigit():
            k += 1
        whole = k - d0
        frac = 0
        if k < n and text[k] == ".":
            k += 1
            f0 = k
            while k < n and text[k].isdigit():
                k += 1
            frac = k - f0
        if whole == 0 and frac == 0:
            return None
        num = text[j:k]
        while k < n and text[k].isspace():
            k += 1
        if k < n and text[k] == ")":
            return float(num), k + 1
        return None

    while i < n:
        c = text[i]
        if c == "\\" and i + 1 < n and text[i + 1] in "()[]\\":
            chars.append([text[i + 1], 1.0])
            i += 2
        elif c == "(" or c == "[":
            opened.append((c, len(chars)))
            i += 1
        elif c == ":" and weight_suffix(i) is not None and last_open("(") is not None:
            w, i = weight_suffix(i)
            mul(opened.pop(last_open("("))[1], w)
        elif c == ")" and last_open("(") is not None:
            mul(opened.pop(last_open("("))[1], 1.1)
            i += 1
        elif c == "]" and last_open("[") is not None:
            mul(opened.pop(last_open("["))[1], 1 / 1.1)
            i += 1
        elif c == ":" and weight_suffix(i) is not None:
            # ``:w)`` with no round bracket open is text as a whole (the ')' does not close anything either)
            end = weight_suffix(i)[1]
            chars.extend([ch, 1.0] for ch in text[i:end])
            i = end
        else:
            chars.append([c, 1.0])
            i += 1
    # brackets still open: round ones first, then square ones, each from where it opened
    for kind, f in (("(", 1.1), ("[", 1 / 1.1)):
        for k, start in opened:
            if k == kind:
                mul(start, f)
    out = []
    for ch, w in chars:
        if out and out[-1][1] == w:
            out[-1][0] += ch
        else:
            out.append([ch, w])
    return [(a, b) for a, b in out] or [("", 1.0)]


def token_stream(tok, prompt, weighting):
    """-> (ids, weights): every fragment tokenised on its own without special tokens."""
    ids, ws = [], []
    for frag, w in (parse_weights(prompt) if weighting else [(prompt, 1.0)]):
        t = list(tok(frag, add_special_tokens=False).input_ids)
        ids += t
        ws += [w] * len(t)
    return ids, ws


def chunk_count(n_tokens, cap):
    return max(1, math.ceil(min(n_tokens, CHUNK * cap) / CHUNK))


def chunk_rows(tok, ids, ws, n):
    """-> ([n][77] ids, [77 n] weights): chunk c = bos + ids + eos + pads, weight 1 on bos / eos / pad; missing chunks empty."""
    rows, weights = [], []
    for c in range(n):
        part, wpart = ids[CHUNK * c:CHUNK * (c + 1)], ws[CHUNK * c:CHUNK * (c + 1)]
        pad = CHUNK - len(part)
        rows.append([tok.bos_token_id] + part + [tok.eos_token_id] + [tok.pad_token_id] * pad)
        weights += [1.0] + wpart + [1.0] * (1 + pad)
    return rows, weights


def apply_weights(z, w):
    """z [77 n, D] of ONE prompt, w [77 n]: untouched when every weight is 1, else scaled and brought back to its mean."""
    w = torch.as_tensor(w, dtype=z.dtype)
    if bool((w == 1).all()):
        return z
    m0 = z.mean()
    z = z * w[:, None]
    return z * (m0 / z.mean())


@torch.no_grad()
def encode(tokenizers, encoders, xl, prompts, max_chunks=1, weighting=False, min_chunks=None):
    """-> (embeds [B, 77 n, D], pooled, n, tokens dropped): every chunk through the encoder ALONE (batch of one row)."""
    if isinstance(prompts, str):
        prompts = [prompts]
    streams = [[token_stream(tok, p, weighting) for p in prompts] for tok in tokenizers]
    cap = CHUNK * max_chunks
    dropped = sum(max(0, max(len(streams[k][b][0]) for k in range(len(tokenizers))) - cap) for b in range(len(prompts)))
    n = max(chunk_count(len(ids), max_chunks) for row in streams for ids, _ in row)
    if min_chunks is not None:
        n = max(n, min_chunks)
    per_encoder, pooled = [], None
    for k, (tok, enc) in enumerate(zip(tokenizers, encoders)):
        outs, first = [], []
        for ids, ws in streams[k]:
            rows, weights = chunk_rows(tok, ids[:cap], ws[:cap], n)
            res = [enc(torch.tensor([r]), output_hidden_states=True) for r in rows]
            z = torch.cat([(r.hidden_states[-2] if xl else r[0])[0] for r in res])
            outs.append((z, apply_weights(z, weights)))
            first.append(res[0][0][0])
        per_encoder.append(outs)
        if xl and k == 1:
            pooled = torch.stack(first)
    if xl:
        embeds = torch.stack([torch.cat([per_encoder[0][b][1], per_encoder[1][b][1]], dim=-1) for b in range(len(prompts))])
    else:
        embeds = torch.stack([o[1] for o in per_encoder[0]])
        pooled = torch.stack([o[0] for o in per_encoder[0]])
    return embeds, pooled, n, dropped
