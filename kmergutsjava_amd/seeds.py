"""Seed sets of the seeded protein search (include/kmerguts_hip.h, kg_proteins_search_seeded): a class map over the twenty
residues and up to four spaced shapes, from their written forms.

An alphabet is `identity`, `reduced11` or GROUPS: comma-separated groups of residue letters, each residue in exactly one group,
the groups numbered in the order written (`AST,C,DEKNQR,F,G,H,ILV,M,P,W,Y` is reduced11).  A shape is a string of `1` (care) and
`0` (don't care), at most 32 long, with the leftmost character as position 0; it begins and ends with `1`.
"""
from __future__ import annotations

from .align_scores import ALPHA

REDUCED11 = "AST,C,DEKNQR,F,G,H,ILV,M,P,W,Y"
ALPHABETS = {"identity": ",".join(chr(c) for c in ALPHA), "reduced11": REDUCED11}
EXACT = dict(alphabet="identity", shapes=["11111111"])
REDUCED = dict(alphabet="reduced11", shapes=["111101101011", "110110011010011"])
BUILTIN = {"exact": EXACT, "reduced": REDUCED}
MAX_SHAPES, MAX_SPAN, MAX_SPACE = 4, 32, 1 << 35


def parse_alphabet(text: str):
    """-> (cls: 20 class numbers in code order ACDEFGHIKLMNPQRSTVWY, the number of classes)."""
    groups = ALPHABETS.get(text, text).split(",")
    letters = bytes(ALPHA).decode()
    cls = {}
    for k, g in enumerate(groups):
        if not g:
            raise ValueError("alphabet %r: group %d is empty" % (text, k))
        for ch in g:
            if ch not in letters:
                raise ValueError("alphabet %r: %r is not one of the residues %s" % (text, ch, letters))
            if ch in cls:
                raise ValueError("alphabet %r: residue %s is in two groups" % (text, ch))
            cls[ch] = k
    missing = [ch for ch in letters if ch not in cls]
    if missing:
        raise ValueError("alphabet %r: residue %s is in no group" % (text, missing[0]))
    if len(groups) < 2:
        raise ValueError("alphabet %r: at least 2 groups are needed" % text)
    return [cls[ch] for ch in letters], len(groups)


def parse_shape(text: str) -> int:
    """-> the mask: bit j set where character j is `1`."""
    if not text or any(ch not in "01" for ch in text):
        raise ValueError("shape %r: a shape is written with the characters 1 and 0" % text)
    if len(text) > MAX_SPAN:
        raise ValueError("shape %r: at most %d positions" % (text, MAX_SPAN))
    if text[0] != "1" or text[-1] != "1":
        raise ValueError("shape %r: the first and the last position must be 1" % text)
    return sum(1 << j for j, ch in enumerate(text) if ch == "1")


def resolve(seeds):
    """None or "exact" -> None (the exact call); "reduced" or a dict(alphabet=..., shapes=[...]) -> (cls, n_classes, masks, the
    alphabet as written, the shapes as written).  A dict may leave out either part: it is then the `exact` set's."""
    if seeds is None or seeds == "exact":
        return None
    if isinstance(seeds, str):
        if seeds not in BUILTIN:
            raise ValueError("seeds must be None, 'exact', 'reduced' or a dict(alphabet=..., shapes=[...])")
        seeds = BUILTIN[seeds]
    unknown = set(seeds) - {"alphabet", "shapes"}
    if unknown:
        raise ValueError("seeds: unknown key %r" % sorted(unknown)[0])
    alphabet = seeds.get("alphabet", EXACT["alphabet"])
    shapes = list(seeds.get("shapes", EXACT["shapes"]))
    if not 1 <= len(shapes) <= MAX_SHAPES:
        raise ValueError("seeds: 1 to %d shapes" % MAX_SHAPES)
    cls, n_cls = parse_alphabet(alphabet)
    masks = [parse_shape(s) for s in shapes]
    weight = bin(masks[0]).count("1")
    for s, m in zip(shapes, masks):
        if bin(m).count("1") != weight:
            raise ValueError("shape %r: %d care positions, shape %r has %d" % (s, bin(m).count("1"), shapes[0], weight))
    if len(masks) * n_cls ** weight > MAX_SPACE:
        raise ValueError("seeds: %d shapes * %d classes ^ weight %d is over 2^35" % (len(masks), n_cls, weight))
    return cls, n_cls, masks, alphabet, shapes


def describe(seeds) -> str:
    """The words the front end's summary line carries: `<alphabet> x <shape,shape>`."""
    _, _, _, alphabet, shapes = resolve(seeds)
    return "%s x %s" % (alphabet, ",".join(shapes))
