"""Inputs and command lines of the drop-in rows: the reference's own command-line tool (`csc c/d`, libcsc/csc.cpp) run over seeded
inputs.  Shared by tools/make_golden_dropin.py (which records what the tool linked to the REFERENCE's libcsc prints and writes:
tests/golden/dropin_cli.json), tests/test_dropin_host.py (the checkers against that record, CPU) and tests/test_gpu_dropin.py (the
same tool linked to the product library, on the GPU)."""
import re

# name -> (input spec in cases.build form, options between `c` and the two file names)
CLI_CASES = {
    # two chunks, so two Progress records; the second chunk is 5 bytes
    "text_2m5_m1_d1m": ([["text", 51, 0, (2 << 20) + 5]], ["-m1", "-d1m"]),
    # the MIX of tests/test_gpu_decode_device.py (280 000 bytes); no -d: the tool clamps the dictionary to the file size (csc.cpp:133-134)
    "mix_m2": ([["text", 21, 0, 150000], ["pattern", "00", 40000], ["exe", 22, 0, 60000], ["zeros", 30000]], ["-m2"]),
    "exe_300k_m3_d64k_noexe": ([["exe", 52, 0, 300000]], ["-m3", "-d64k", "-fexe0"]),
    "delta_200k_m4_notxt_nodelta": ([["delta", 53, 0, 200000]], ["-m4", "-ftxt0", "-fdelta0"]),
    # dictionary smaller than the input
    "silesia_600k_m5_d256k": ([["silesia", 54, 0, 600000]], ["-m5", "-d256k"]),
    "random_40k_m3": ([["random", 55, 0, 40000]], ["-m3"]),
    "one_byte": ([["pattern", "78", 1]], []),
    "empty": ([], []),
}

IN_NAME, OUT_NAME, BACK_NAME = "in.bin", "out.csc", "back.bin"


def encode_argv(case):
    return ["c"] + CLI_CASES[case][1] + [IN_NAME, OUT_NAME]


def decode_argv():
    return ["d", OUT_NAME, BACK_NAME]


def props_of(lib, case, n):
    """the CSCProps csc.cpp:125-142 builds for the case's options over an input of n bytes, through `lib` (a capi.CscLib)"""
    level, dict_size = 2, 64000000
    for o in CLI_CASES[case][1]:
        if o.startswith("-m"):
            level = int(o[2:])
        elif o.startswith("-d"):
            dict_size = int(o[2:-1]) << {"k": 10, "m": 20}[o[-1]]
    p = lib.props_init(min(dict_size, n), level)
    for o in CLI_CASES[case][1]:
        if o == "-fdelta0":
            p.DLTFilter = 0
        elif o == "-fexe0":
            p.EXEFilter = 0
        elif o == "-ftxt0":
            p.TXTFilter = 0
    return p


_REC = re.compile(r"\r(\d+) -> (\d+)\t\t\t\t")


def parse_stderr(text):
    """-> (MB of the "Estimated memory usage" line or None, [(in, out), ...] of the `\\r%llu -> %llu` records); the whole text must be
    made of these and nothing else (csc.cpp:35,144)"""
    mem = None
    m = re.match(r"Estimated memory usage: (\d+) MB\n", text)
    if m:
        mem = int(m.group(1))
        text = text[m.end():]
    pairs = [(int(a), int(b)) for a, b in _REC.findall(text)]
    assert _REC.sub("", text) == "", repr(text[:200])
    return mem, pairs
