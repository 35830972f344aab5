"""Greedy speculative decoding on top of `DecodeStack.verify`: a cheap drafter proposes k tokens per sequence, the target scores the
last real token and the k drafts in ONE pass (k + 1 <= 8 rows per sequence on the split-KV verify attention kernel) and keeps the prefix
it agrees with, plus its own next token -- so every round emits between 1 and k + 1 tokens that are exactly the target's greedy choice.

Acceptance is greedy (arg-max agreement) only; sampling-based acceptance (rejection sampling against the drafter's distribution) is out
of scope here."""
from __future__ import annotations

import torch


def accept_greedy(draft: torch.Tensor, target_argmax: torch.Tensor):
    """draft [n, T]: column 0 is the last real token of each sequence, columns 1 ... T - 1 the proposed tokens; target_argmax [n, T]: the
    arg-max of the target's logits behind each of those T tokens.  Returns (accepted [n], next_token [n]): the length of the longest prefix
    with target_argmax[:, t] == draft[:, t + 1], and the target's arg-max behind that prefix (the token the target itself emits next).
    Plain torch on whatever device the inputs live on; nothing is read on the host."""
    if draft.shape != target_argmax.shape or draft.dim() != 2 or draft.shape[1] < 1:
        raise ValueError(f"draft and target_argmax must both be [n, T >= 1], got {tuple(draft.shape)} and {tuple(target_argmax.shape)}")
    agree = (target_argmax[:, :-1] == draft[:, 1:]).long()
    accepted = agree.cumprod(dim=1).sum(dim=1)
    return accepted, target_argmax.gather(1, accepted.view(-1, 1)).squeeze(1)


def _stack_drafter(draft):
    """A ragged DecodeStack as drafter: `prime(prompt)` fills its cache, `propose(tok, pos, k)` decodes greedily from the last real tokens
    `tok` [bs] at host positions `pos`.  It feeds k + 1 tokens (the k-th draft too), so its cache holds a row for every token the target
    may accept; rewinding it after a rejection is nothing but the next call's smaller positions: rows above them are dead."""
    if not draft.ragged or draft.lm_head is None:
        raise ValueError("a DecodeStack drafter must be built with ragged=True and an LM head")

    def prime(prompt):
        draft.prefill(prompt, position=0)

    def propose(seqs, tok, pos, k):
        out = []
        for j in range(k + 1):
            tok = draft.decode(tok, [p + j for p in pos]).argmax(-1)
            out.append(tok.clone())
        return torch.stack(out[:k], dim=1)

    return prime, propose


@torch.no_grad()
def generate_speculative(stack, draft, prompt: torch.Tensor, new_tokens: int, k: int):
    """Greedy continuation of `prompt` [bs, L] by `new_tokens` tokens per sequence, k drafts per round (1 <= k <= 7).
    stack: the target, a ragged DecodeStack with an LM head.  draft: a second ragged DecodeStack of the same batch size (its own weights
    and cache), or any callable (seqs, k) -> int64 [bs, k], where seqs is the list of each sequence's tokens so far (prompt + output, 1-D).
    A round: verify [last token, k drafts] -> accept_greedy -> every sequence advances by accepted + 1 positions -> the drafter is rewound
    to the new positions.  Rejected drafts leave dead cache rows above the new position (DecodeStack.verify).  A sequence that has its
    new_tokens stops advancing.  Returns (tokens [bs, new_tokens], mean accepted drafts per sequence and round).
    The tokens are the target's own greedy choices up to the numeric contract between `verify` and `decode` logits."""
    T = k + 1
    if not 1 <= k <= 7:
        raise ValueError(f"k must be in 1 ... 7 (a verify pass scores k + 1 <= 8 tokens), got {k}")
    if not stack.ragged or stack.lm_head is None:
        raise ValueError("generate_speculative needs a target built with ragged=True and an LM head")
    if prompt.dim() != 2 or prompt.shape[0] != stack.bs or prompt.shape[1] < 1 or new_tokens < 1:
        raise ValueError(f"prompt must be [bs = {stack.bs}, L >= 1] and new_tokens >= 1")
    bs, L = prompt.shape
    if L + new_tokens + T > stack.cfg.max_seq:
        raise ValueError(f"prompt {L} + new_tokens {new_tokens} + k + 1 = {T} exceeds the KV cache ({stack.cfg.max_seq})")
    dev = prompt.device
    prime, propose = _stack_drafter(draft) if hasattr(draft, "decode") else (None, lambda seqs, tok, pos, kk: draft(seqs, kk).to(dev))
    tok = stack.prefill(prompt, position=0).argmax(-1)   # the first emitted token; it is fed at position L
    if prime is not None:
        prime(prompt)
    cap = new_tokens + T
    out = torch.zeros(bs, cap + 1, dtype=torch.long, device=dev)  # (column `cap` takes what a round writes beyond a sequence's share)
    out[:, 0] = tok
    cnt = torch.ones(bs, dtype=torch.long, device=dev)            # tokens emitted per sequence
    col = torch.arange(T, device=dev).view(1, T)
    accepted_sum, rounds = 0, 0
    while True:
        counts = cnt.tolist()
        if min(counts) >= new_tokens:
            break
        pos = [L + min(c, new_tokens) - 1 for c in counts]       # where each sequence's last emitted token is fed (finished: inside the cache)
        seqs = [torch.cat([prompt[b], out[b, :counts[b]]]) for b in range(bs)] if prime is None else None
        drafts = torch.cat([tok.view(bs, 1), propose(seqs, tok, pos, k)], dim=1)  # [bs, T]
        acc, nxt = accept_greedy(drafts, stack.verify(drafts, pos).argmax(-1))
        live = cnt < new_tokens
        acc = torch.where(live, acc, torch.full_like(acc, -1))   # (a finished sequence emits nothing and stays where it is)
        emit = torch.cat([drafts[:, 1:], nxt.view(bs, 1)], dim=1).scatter(1, acc.clamp_min(0).view(bs, 1), nxt.view(bs, 1))
        where = torch.where(col <= acc.view(bs, 1), (cnt.view(bs, 1) + col).clamp_max(cap), torch.full_like(col, cap))
        out.scatter_(1, where, emit)
        cnt = cnt + acc + 1
        tok = torch.where(live, nxt, tok)
        accepted_sum += int(acc.clamp_min(0).sum())
        rounds += int(live.sum())
    return out[:, :new_tokens].contiguous(), accepted_sum / max(rounds, 1)
