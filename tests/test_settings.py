"""A handle's settings live in one record with one table (msckf_mono_amd/csrc/settings.h): defaults, environment variables,
the one value check, what a copy takes over.  The header is checked on its own by a stand-alone program
(tests/cpp/settings_host.cpp, g++; once more under the address and undefined-behaviour sanitizers, run directly); here, beside
that, the table of INTEGRATION.md names the same variables as the header, and the library reads the environment nowhere else."""
import glob
import os
import re
import subprocess

import pytest

import helpers as H

ROOT = H.ROOT
CSRC = os.path.join(ROOT, "msckf_mono_amd", "csrc")
PROCESS_WIDE = {"MSCKF_HIP_ROCTX", "MSCKF_HIP_HOST_THREADS", "MSCKF_HIP_CYCLE_TIMERS"}


def _header_variables():
    text = open(os.path.join(CSRC, "settings.h")).read()
    table = text[text.index("SETTINGS_TABLE[] = {"):]
    table = table[:table.index("};")]
    return re.findall(r'\{"(MSCKF_HIP_[A-Z_]+)"', table)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]], ids=["plain", "sanitized"])
def test_settings_header_alone(tmp_path, flags):
    exe = str(tmp_path / "settings_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "settings_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True)      # (the program clears the variables of the table itself)
    assert run.returncode == 0 and run.stdout.strip() == "settings ok", (run.returncode, run.stdout, run.stderr)


def test_integration_table_names_the_variables_of_the_header():
    names = _header_variables()
    assert len(names) == len(set(names)) == 12 and PROCESS_WIDE <= set(names), names
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = text.index("| variable | setter | default | read | copy |")
    rows = text[start:text.index("\n\n", start)].splitlines()[2:]
    assert all(r.startswith("|") and r.count("|") >= 6 for r in rows), rows
    first = [r.split("|")[1].strip() for r in rows]
    documented = [m.group(0) for cell in first for m in [re.fullmatch(r"`(MSCKF_HIP_[A-Z_]+)`", cell)] if m]
    documented = [d.strip("`") for d in documented]
    assert all(cell == "—" or cell.strip("`") in documented for cell in first), first
    assert sorted(documented) == sorted(names)
    # process-wide variables say so in the column "read", the others are read when the handle is created
    for r in rows:
        cells = [c.strip() for c in r.split("|")]
        if cells[1] != "—":
            assert cells[4].startswith("process-wide") == (cells[1].strip("`") in PROCESS_WIDE), r
            assert cells[1].strip("`") in PROCESS_WIDE or cells[4] == "create", r


def test_the_library_reads_the_environment_in_the_table_and_at_three_named_places():
    found = {}
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(sources) >= 13, sources
    for path in sources:
        lines = [ln.strip() for ln in open(path).read().splitlines() if "getenv" in ln]
        if lines:
            found[os.path.basename(path)] = lines
    assert sorted(found) == ["msckf_hip.hip", "settings.h"], found
    assert len(found["settings.h"]) == 1 and "getenv(r.env)" in found["settings.h"][0], found["settings.h"]
    named = [re.findall(r'getenv\("([A-Z_]+)"\)', ln) for ln in found["msckf_hip.hip"]]
    assert all(len(n) == 1 for n in named), found["msckf_hip.hip"]
    assert sorted(n[0] for n in named) == sorted(PROCESS_WIDE), found["msckf_hip.hip"]
