"""What `csarc a` would find on disk for a case of tests/csa_cases.py, as the table CSAMI_DeviceWrite takes -- with no tree on disk.
Shared by tests/test_archive_device_write_host.py (the planner) and tests/test_gpu_archive_device_write.py (the archives)."""
import os

import cases
import csa_cases

FILE_ATTR = ord("u") + (0o100644 << 8)
DIR_ATTR = ord("u") + (0o040755 << 8)


def spec_size(parts):
    return sum(p[3] for p in parts)


def scanned(case):
    """-> [(name, parts or None for a directory)] in the order of no particular meaning: the entries scandir (csarc.cpp:709-750)
    adds for the case's arguments"""
    spec = csa_cases.CSA_CASES[case]
    out = {}
    for arg in spec["args"]:
        if arg in spec["files"]:
            out[arg] = spec["files"][arg]
            continue
        out[arg + "/"] = None
        if not spec["opts"].get("recurse"):
            continue
        for rel, parts in spec["files"].items():
            if not rel.startswith(arg + "/"):
                continue
            out[rel] = parts
            d = os.path.dirname(rel)
            while d and d != arg:
                out[d + "/"] = None
                d = os.path.dirname(d)
    return list(out.items())


def table(case, edate, with_bytes=True, residue=0):
    """-> ([{name, esize, edate, eattr, offset}], the source bytes (None without with_bytes: the planner reads no byte),
    {name: content}).  Every file starts `residue` bytes behind a multiple of 16."""
    files, src, content, pos = [], bytearray(), {}, 0
    for name, parts in scanned(case):
        if parts is None:
            files.append({"name": name, "esize": 0, "edate": edate, "eattr": DIR_ATTR, "offset": 0})
            continue
        n = spec_size(parts)
        off = (pos + 15) // 16 * 16 + residue
        files.append({"name": name, "esize": n, "edate": edate, "eattr": FILE_ATTR, "offset": off})
        if with_bytes:
            content[name] = cases.build(parts) if parts else b""
            src += bytes(off - pos) + content[name]
        pos = off + n
    return files, (bytes(src) if with_bytes else None), content
