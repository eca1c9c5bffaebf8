"""Writes tests/golden/txkeyer.npz: the keyer's named cases (tests/txkeyer_cases.py) with the key bytes and the end state that the law
gives them.  The reference has the paddles' pins and no keyer (include/selenite_tx_keyer.h), so the expected values come from the oracle
(tests/txkeyer_oracle.py) -- and are written only if its two statements of the law, sample by sample and over run lengths, agree on every
byte and every state word.

    python tests/golden/make_txkeyer_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import txkeyer_cases as kc  # noqa: E402
import txkeyer_oracle as ko  # noqa: E402


def main():
    out = {"names": np.array(sorted(kc.CASES))}
    for name in sorted(kc.CASES):
        a, b = kc.OracleBackend(False), kc.OracleBackend(True)
        ka, kb = kc.play(kc.CASES[name], a), kc.play(kc.CASES[name], b)
        sa, sb = a.state(), b.state()
        if not np.array_equal(ka, kb) or any(not np.array_equal(sa[w], sb[w]) for w in sa):
            raise SystemExit("%s: the two statements of the law disagree; nothing written" % name)
        out[name + "/key"] = ka
        out[name + "/words"] = np.stack([sa[w] for w in ko.WORDS])
        out[name + "/text"] = sa["text"]
    path = os.path.join(HERE, "txkeyer.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(kc.CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
