#!/usr/bin/env python3
"""Writes tests/golden/reference_wordpiece.json: a generated vocabulary, generated rows and the ids an independent CPU
implementation gives them -- the `tokenizers` library's WordPiece model under WhitespaceSplit (punct = 0) and under
BertPreTokenizer (punct = 1).  The tests read the file and never import that library.

That library splits on Unicode whitespace and punctuation, the definition (custrings_amd/csrc/wordpiece_ops.h) on bytes
<= 0x20 and ASCII punctuation: the rows use only space, \\t, \\n, \\r, \\x0b, \\x0c as whitespace, no other byte below 0x20, no
non-ASCII punctuation or whitespace, and are well-formed UTF-8 (asserted below).

    python tools/make_wordpiece_golden.py [--check]      # --check: compare with the committed file, write nothing
"""
import json
import os
import sys
import unicodedata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wordpiece_model as m  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "reference_wordpiece.json")
PREFIX, UNK = "##", "[UNK]"
# (punct, max_word_chars): the default, and limits at and around the rows' word lengths (1..8 characters)
CASES = [(0, 100), (1, 100), (0, 6), (0, 5), (0, 1), (1, 4), (1, 3)]
ALLOWED_BLANKS = set(" \t\n\r\x0b\x0c")


def check_inputs(texts):
    for t in texts:
        for ch in t:
            if ch in ALLOWED_BLANKS or ord(ch) < 0x80 and ord(ch) > 0x20:
                continue
            assert ord(ch) >= 0x80, "a control byte in the fixture's rows: %r" % t
            cat = unicodedata.category(ch)
            assert not cat.startswith("P") and not cat.startswith("Z") and not ch.isspace(), "non-ASCII punctuation or whitespace: %r" % t


def reference_ids(vocab, texts, punct, max_word_chars):
    from tokenizers import Tokenizer, models, pre_tokenizers

    ids = {}
    for i, e in enumerate(vocab):
        ids.setdefault(e, i)
    tok = Tokenizer(models.WordPiece(vocab=ids, unk_token=UNK, max_input_chars_per_word=max_word_chars, continuing_subword_prefix=PREFIX))
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer() if punct else pre_tokenizers.WhitespaceSplit()
    return [enc.ids for enc in tok.encode_batch(texts, add_special_tokens=False)]


def generate():
    vocab = [e.decode() for e in m.make_vocab(300, 11)]
    assert len(set(vocab)) == len(vocab) and all(e.encode() in set(v.encode() for v in vocab) for e in ("##", "#", "###", "##a#", "a##b"))
    texts = [r.decode() for r in m.make_rows(480, 12)]
    texts += ["", " ", "\t\n", "##ab", "##", "###", "####", "##a#", "a##b", "#a ##a a## a#a", "[UNK]", "[UNK]a", "a,b", ",", ",,", " , ",
              "abcde", "abcdef", "abcdefg", "語語語語語", "語語語語語語", "😀😀😀😀", "a😀", "😀", "ab" * 30]
    check_inputs(texts)
    cases = []
    for punct, mwc in CASES:
        ids = reference_ids(vocab, texts, punct, mwc)
        flat = [i for row in ids for i in row]
        share = flat.count(vocab.index(UNK)) / len(flat)
        if mwc == 100:  # (the small limits turn most words into unk on purpose)
            assert 0.02 <= share <= 0.30, "the unk share of the fixture is %.3f: one of the two branches goes untested" % share
        cases.append({"punct": punct, "max_word_chars": mwc, "unk_share": round(share, 4), "ids": ids})
    return {"prefix": PREFIX, "unk": UNK, "library": "tokenizers 0.22.2", "vocab": vocab, "rows": texts, "cases": cases}


def dumps(doc):
    head = {k: v for k, v in doc.items() if k != "cases"}
    lines = [json.dumps(head, ensure_ascii=True)[:-1] + ', "cases": [']
    for i, c in enumerate(doc["cases"]):
        lines.append(json.dumps(c, ensure_ascii=True, separators=(",", ":")) + ("," if i + 1 < len(doc["cases"]) else ""))
    lines.append("]}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = dumps(generate())
    if "--check" in sys.argv[1:]:
        sys.exit(0 if open(PATH).read() == text else "the committed fixture differs from what the library gives now")
    open(PATH, "w").write(text)
    print("%s: %d bytes" % (PATH, len(text)))
