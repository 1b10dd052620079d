"""Sheets and classes for the cascade with layer numbers local to a class (OSMT_RULES_CLASS_LAYERS), shared by
tests/test_cascade_layers_cpu.py (the mirror against the Python restatement) and tests/test_gpu_cascade_layers.py (the device
against the mirror).  Every rule has ONE selector, so selector i is rule i, and a class is (slot, layer tag, [selector ids])
as in tests/_cascade.py.  The set-wide number of a layer is its rank by first use in selector order."""
from osm_renderer_amd import abi
from tests._cascade import nums, sel

# the layer names of the reference's mapnik sheet, typed in (None: "default")
REF_NAMES = [None, "*", "bridge-casing1", "bridge-casing2", "over1", "over2", "over3", "over4", "over5", "over6", "oneway", "oneway_over1", "oneway_over2",
             "oneway_over3", "roads-casing", "casing1", "casing2", "access", "under1", "under2", "water_lines-casing", "turning_circle-casing", "tram",
             "tram_under2", "tram_under3", "ele"]
assert len(set(REF_NAMES)) == len(REF_NAMES) == 26
NUMBERS = (0, 7, 8, 31, 32, 63, 64, 127, 128, 254)  # set-wide numbers at the edges of a byte's and a word's bits


def props_of(k, layer):
    """the properties of rule k.  What is always read: a width of its own (a rule of "*": opacity, colour and line cap, so that
    its writes show), on every fourth rule a text with a font size.  Behind them every name and every kind of value comes
    round (the generator of tests/test_gpu_cascade.test_selector_counts_and_layers_per_class, held below its 300 rules)"""
    k %= 300
    values = [nums(float(k)), ("id", "round"), ("color", (k % 256, 1, 2)), ("delta", 0.5), nums(1, k)]
    if layer == "*":
        seen = [("opacity", nums((k % 4 + 1) * 0.25)), ("color", ("color", (k % 256, 2, 3))), ("linecap", ("id", "round"))]
    else:
        seen = [("width", nums(1.0 + k * 0.5))]
    if k % 4 == 1:
        seen += [("text", ("id", "name")), ("font-size", nums(8.0 + k % 5))]
    return seen + [(abi.PROP_NAMES[(k + j) % 20], values[(k + j) % 5]) for j in range(1 + k % 3)]


def rules_of(order):
    """[(layer, lo, hi)] -> a sheet, one rule and one selector per entry"""
    return [([sel(layer, lo, hi)], props_of(k, layer)) for k, (layer, lo, hi) in enumerate(order)]


def names_of(n):
    """n distinct names; "*" is number 1, but in the sheet of 255 it is the LAST name: the highest set-wide number, 254"""
    if n <= 26:
        return REF_NAMES[:n]
    return [None] + [f"n{k}" for k in range(1, n - 1)] + ["*"]


def names_case(n):
    """rule k names layer k (k < n), with zoom bounds on some; selector n is one more "*" from zoom 10.  Classes: every number of
    NUMBERS the sheet has alone, with its neighbour, under "*" and before the late "*"; all of them together; the 16 highest"""
    names = names_of(n)
    star = names.index("*")
    order = [(nm, k % 5 if k % 3 == 0 and k else None, 18 - k % 7 if k % 4 == 0 and k else None) for k, nm in enumerate(names)] + [("*", 10, None)]
    marks = sorted({t for t in NUMBERS if t < n} | {n - 1})
    classes = []
    for i, t in enumerate(marks):
        classes.append((2, None, [t]))
        classes.append((1, i, sorted({t, min(t + 1, n - 1)})))
        classes.append((2, None, sorted({star, t})))
        classes.append((3, None, [t, n]))
    classes.append((2, None, sorted(set(marks) | {star})))
    classes.append((2, 1, sorted(set(marks) | {star, n})))
    classes.append((2, None, sorted(set(range(max(0, n - 16), n)))))
    return rules_of(order), classes


# ---- layers per class -------------------------------------------------------------------------------------------
# 0 "default" implied; 1 "*"; 2 .. 13 twelve names; 14 "*" again, in the middle; 15 .. 26 twelve more names; 27 "*" at zooms 8 .. 12
# only; 28 ::default spelled out; 29, 30 two names again, met in the opposite order; 31 "default" implied, zooms 3 .. 9; 32 "*" last
LAYER_ORDER = ([(None, None, None), ("*", None, None)] + [(nm, None, None) for nm in REF_NAMES[2:14]] + [("*", None, None)] +
               [(nm, None, 18 - k) if k % 3 == 0 else (nm, None, None) for k, nm in enumerate(REF_NAMES[14:26])] +
               [("*", 8, 12), ("default", None, None), ("over1", None, None), ("bridge-casing1", 5, None), (None, 3, 9), ("*", None, None)])
PLAIN = [0] + list(range(2, 14)) + list(range(15, 27))  # 25 selectors of 25 distinct layers, no "*"


def layers_case():
    classes = [(2, None, PLAIN[:k]) for k in range(1, 17)]            # 1 .. 16 layers, "*" absent
    classes += [
        (1, None, [1] + PLAIN[1:6]),                                   # "*" first
        (1, None, [0, 2, 3, 14, 15, 16]),                              # in the middle: 15 and 16 are created after it and copy it
        (1, None, [0, 2, 3, 32]),                                      # last
        (1, None, [0, 2, 27]), (1, None, [0, 2, 27, 30]),              # admitted at zooms 8 .. 12 only, last and before a new layer
        (1, None, [27]), (1, None, [1]),                               # "*" alone: no style
        (3, None, [1] + PLAIN[1:16]),                                 # 16 layers with "*" first,
        (3, None, PLAIN[:7] + [14] + PLAIN[13:21]),                    # ... in the middle,
        (3, None, PLAIN[:15] + [32]),                                  # ... last,
        (3, 2, [1] + PLAIN[1:8] + [14] + PLAIN[13:20] + [27, 32]),      # ... and four times
        (2, None, [0, 28]), (2, None, [28]), (2, None, [2, 28, 31]), (2, 0, [31]),  # "default" spelled out and implied
        (2, None, [1, 5]), (2, None, [14, 20]), (2, None, [0, 14, 20, 32]),          # a layer created after "*"
        (2, None, [2, 4]), (2, None, [29, 30]), (2, None, [4, 30]), (2, None, [1, 2, 4, 29, 30]),  # the same two layers, met in opposite order
        (0, None, []),
    ]
    assert all(sels == sorted(sels) for _, _, sels in classes)  # a match lists a class's selectors ascending
    return rules_of(LAYER_ORDER), classes


def long_case():
    """255 names, then 300 rules cycling over 16 of them; a class of those 300 selectors and one of every third"""
    names = names_of(255)
    pick = [0, 254, 7, 8, 31, 32, 63, 64, 127, 128, 253, 100, 200, 2, 3, 4]
    order = [(nm, None, None) for nm in names] + [(names[pick[k % 16]], k % 19 if k % 5 == 0 else None, None) for k in range(300)]
    return rules_of(order), [(2, None, list(range(255, 555))), (1, None, list(range(255, 555, 3))), (2, None, [254] + list(range(300, 316)))]


def layer_count(sheet, sels):
    """the distinct layers the selectors name, "*" and "default" counted"""
    flat = [s[4] or "default" for ss, _ in sheet for s in ss]
    return len({flat[i] for i in sels})
