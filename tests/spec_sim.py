"""The prompt-lookup drafter and the speculative loop of q3_generate_lookup restated in plain Python (include/qwen3_hip.h
section 2c).  The tests hold the library against these: the drafter token for token, the loop's four statistics exactly."""


def draft_ref(S, ngram, draft_len):
    """Largest i < |S| - g with S[i:i+g] == S[-g:]; the draft is S[i+g : i+g+draft_len].  [] = no draft."""
    g, n = ngram, len(S)
    if g < 1 or draft_len < 1 or n <= g:
        return []
    for i in range(n - g - 1, -1, -1):
        if S[i:i + g] == S[n - g:]:
            return list(S[i + g:i + g + draft_len])
    return []


def simulate(G, corpus, first_token, ngram, draft_len):
    """Replay q3_generate_lookup against the reference tokens G (= generate_greedy(first_token, p0, len(G))): draft from
    S = corpus ++ [first_token] ++ generated, cut the draft so that a round yields no more tokens than are still wanted,
    accepted = length of the draft's common prefix with G.  Returns the statistics and, per pass, (drafted, accepted)."""
    S = list(corpus) + [first_token]
    k, passes, single, drafted, accepted = 0, [], 0, 0, 0
    while k < len(G):
        d = draft_ref(S, ngram, draft_len)[:len(G) - k - 1]
        if not d:
            S.append(G[k])
            k += 1
            single += 1
            continue
        a = 0
        while a < len(d) and d[a] == G[k + a]:
            a += 1
        passes.append((len(d), a))
        drafted += len(d)
        accepted += a
        S.extend(G[k:k + a + 1])
        k += a + 1
    return {"verify_passes": len(passes), "single_steps": single, "drafted": drafted, "accepted": accepted, "passes": passes}
