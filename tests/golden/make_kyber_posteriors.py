#!/usr/bin/env python3
"""Mint tests/golden/kyber_posteriors.json from the reference's simulate/max_likelihood.py (which imports nothing but
itertools): for codings of this project's own making, Pr[y | symbol] (pr_cond_yx) for every oracle answer y and the posterior
s_distribution_from_hard_y hands the decoder for it.  Only the inputs and the resulting numbers are stored (float64, as
repr round-trips them).

    python tests/golden/make_kyber_posteriors.py <reference checkout>/simulate-with-python

An answer whose probability is 0 under every symbol makes the reference divide by zero; it is stored under "dropped".
"""
import importlib.util
import itertools
import json
import os
import sys
from math import comb

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kyber_posteriors.json")


def expansion(symbols, bits):
    return [tuple((s >> (bits - 1 - i)) & 1 for i in range(bits)) for s in range(symbols)]


def binomial_law(B):
    return [comb(2 * B, q) / 2 ** (2 * B) for q in range(2 * B + 1)]


CODINGS = {
    "parity_1bit_5": ([(s & 1,) for s in range(5)], 2),
    "expansion_3bit_5": (expansion(5, 3), 2),
    "expansion_4bit_13": (expansion(13, 4), 6),
}
POSITIONAL = [(0.1, 0.05), (0.02, 0.2), (0.0, 0.3), (0.15, 0.01)]


def main(ref):
    spec = importlib.util.spec_from_file_location("max_likelihood", os.path.join(ref, "simulate", "max_likelihood.py"))
    ml = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ml)
    cases = []
    for name, (code, B) in CODINGS.items():
        P = len(code[0])
        prior = binomial_law(B)
        coding = {s: code[s + B] for s in range(-B, B + 1)}
        distrib = {s: prior[s + B] for s in range(-B, B + 1)}
        for accuracy in (1.0, 0.95, POSITIONAL[:P]):
            oracle = ml.SimpleOracle(accuracy) if isinstance(accuracy, float) else ml.FalsePositiveNegativePositionalOracle(accuracy)
            answers, dropped, weights, levels = [], [], [], []
            for y in itertools.product(range(2), repeat=P):
                cond = [ml.pr_cond_yx(y, coding[s], oracle) for s in range(-B, B + 1)]
                try:
                    post = ml.s_distribution_from_hard_y(y, oracle, lambda sw: range(-B, B + 1), coding, distrib, 1)
                except ZeroDivisionError:
                    assert not any(cond)
                    dropped.append(list(y))
                    continue
                answers.append(list(y))
                weights.append([float(c) for c in cond])
                levels.append([float(p) for p in post])
            cases.append(dict(name=name, coding=[list(c) for c in code], prior=prior,
                              accuracy=accuracy if isinstance(accuracy, float) else [list(p) for p in accuracy], answers=answers,
                              dropped=dropped, weights_by_answer=weights, levels=levels))
    with open(OUT, "w") as fh:
        json.dump(dict(cases=cases), fh, indent=1)
        fh.write("\n")
    print(f"{OUT}: {len(cases)} cases")


if __name__ == "__main__":
    main(sys.argv[1])
