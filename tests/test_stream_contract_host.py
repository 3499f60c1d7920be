"""The table of the stream contract, without a device (include/diffab_hip.h, "Streams"; tests/test_gpu_stream_contract.py).

Every export of every header is in exactly one of three sets: DRIVEN under the gate by a named row of the GPU test, ENQUEUES_NOTHING
(queries, setters, host-only diagnostics: there is nothing to put on a stream) or EXEMPT with a reason.  A new export in no set fails
here.  Every parameter or struct field the headers call HOST is a row of the HOST-array test or listed with the reason why it needs
none, and the `stream` parameter the harness replaces is the one ctypes passes.
"""
import ctypes as C
import os
import re

from conftest import REPO
from sampler_support import (ALL_HEADERS, DIAGNOSTIC_HEADERS, ENTRIES, HEADERS, HOST_ARRAYS, HOST_NOT_ARRAYS, LATER_HEADERS, MAY_WAIT, NO_DATA,
                             all_argtypes, all_writes, header_exports, header_prototypes)

# Nothing is enqueued: version and error strings, the device query, switches of process-wide state, size queries, and the launch-form
# query that runs on the host alone.
ENQUEUES_NOTHING = {n for n, c in ENTRIES.items() if c == NO_DATA} - {"diffab_kernel_timer_read"}
EXEMPT = {
    "diffab_kernel_timer_read": "waits for the timer's events by design (hipEventSynchronize): the one documented host wait of a diagnostic",
    "diffab_debug_start_classes": "diagnostic header without a ctypes table; on_device = 0 runs on the host, on_device != 0 enqueues the "
                                  "launch the sample loop's own rows drive (launch_start_classes)",
}


def test_every_export_is_driven_enqueues_nothing_or_is_exempt():
    from test_gpu_stream_contract import DRIVEN, DROPPED, ROWS
    from test_gpu_operand_extents import CASES

    assert sorted(os.listdir(os.path.join(REPO, "include"))) == sorted(ALL_HEADERS + DIAGNOSTIC_HEADERS)  # a new header fails here
    assert len(ALL_HEADERS) == 9 and ALL_HEADERS == HEADERS + LATER_HEADERS
    product, diagnostic = header_exports(ALL_HEADERS), header_exports(DIAGNOSTIC_HEADERS)
    assert sorted(all_argtypes()) == product  # every export of the nine headers has its ctypes signature
    assert len(product) == 107 and diagnostic == ["diffab_debug_start_classes"]
    exports = set(product) | set(diagnostic)
    sets = {"driven": set(DRIVEN), "enqueues nothing": ENQUEUES_NOTHING, "exempt": set(EXEMPT)}
    for a in sets:
        for b in sets:
            assert a == b or not sets[a] & sets[b], (a, b, sorted(sets[a] & sets[b]))
    classified = set().union(*sets.values())
    assert classified == exports, (sorted(exports - classified), sorted(classified - exports))
    assert all(EXEMPT.values()) and set(MAY_WAIT) <= set(DRIVEN) and all(why for _, why in MAY_WAIT.values())
    # an entry that enqueues nothing has no stream to be handed; every other export has exactly one, and it is the last parameter
    protos = header_prototypes(ALL_HEADERS + DIAGNOSTIC_HEADERS)[1]
    for name in exports:
        has = [p[0] for p in protos[name]].count("stream")
        assert has == (0 if name in ENQUEUES_NOTHING or name == "diffab_kernel_timer_read" else 1), (name, has)
    # rows are dropped, entries are not: a dropped row names the row of the same entries that stays
    for row, stays in DROPPED.items():
        assert row in CASES and stays in ROWS and set(CASES[row][0]) <= set(ROWS[stays][0]), (row, stays)
    assert len(LATER_HEADERS) == 7 and len(header_exports(LATER_HEADERS)) == 12 and set(header_exports(LATER_HEADERS)) <= set(DRIVEN)


def test_the_stream_parameter_of_the_prototypes_is_the_one_ctypes_passes():
    from test_gpu_stream_contract import DRIVEN

    protos, argtypes, writes = header_prototypes(ALL_HEADERS)[1], all_argtypes(), all_writes()
    for entry in DRIVEN:
        names = [p[0] for p in protos[entry]]
        at = names.index("stream")
        assert len(names) == len(argtypes[entry]) and at == len(names) - 1 and argtypes[entry][at] is C.c_void_p, entry
        assert protos[entry][at][1:] == ("void", True, False), (entry, protos[entry][at])  # void* stream
        assert entry in writes and "stream" not in writes[entry].split(), entry


def host_words():
    """The identifier in front of every `HOST` of the headers' text (comments included): `ctx_of_row is a HOST array`, `slot_of_step[t]
    (a HOST table`, `const int32_t* steps; /* HOST (n_steps)`, `point_radius (HOST float[P])`."""
    found = set()
    for h in ALL_HEADERS + DIAGNOSTIC_HEADERS:
        text = open(os.path.join(REPO, "include", h)).read()
        for m in re.finditer(r"\bHOST\b", text):
            before = re.sub(r"\[[A-Za-z0-9_ +*-]{0,12}\]", "", text[max(0, m.start() - 120):m.start()])  # (slot_of_step[t] -> slot_of_step)
            words = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", before)
            while words and words[-1] in ("is", "are", "a", "an", "and", "the", "out"):  # (`plan and out are HOST memory`)
                words.pop()
            found.add(words[-1])
    return found


def test_every_host_parameter_has_an_overwrite_case_or_a_reason():
    from test_gpu_stream_contract import HOST_ARRAY_TESTS

    HOST_ARRAY_TESTS()  # every row of HOST_ARRAYS names its test
    structs, protos = header_prototypes(ALL_HEADERS + DIAGNOSTIC_HEADERS)
    # the rows name real operands: a pointer to const, as a parameter or behind the struct path
    for entry, operand in HOST_ARRAYS:
        path = operand.split(".")
        params = {p[0]: p for p in protos[entry]}
        name, base, pointer, const = params[path[0]]
        for field in path[1:]:
            name, base, pointer, const = {f[0]: f for f in structs[base]}[field]
        assert pointer and const and base in ("int32_t", "float"), (entry, operand, base, pointer, const)
    for (owner, name), why in HOST_NOT_ARRAYS.items():
        fields = structs[owner] if owner in structs else protos[owner]
        assert why and name in [f[0] for f in fields], (owner, name)
    named = {operand.split(".")[-1] for _, operand in HOST_ARRAYS} | {name for _, name in HOST_NOT_ARRAYS}
    # `jump coefficients (HOST tables` is beta_jump / alpha_jump in words
    words = host_words() - {"coefficients"}
    assert words == named, (sorted(words - named), sorted(named - words))
