"""The owners of streams, events and cached arenas (csrc/mi_own.h), checked on the host."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (own_test.cpp is clean under -fsanitize=thread as well; that build is no variant here because the thread sanitizer's runtime refuses
# to start under some hosts' address-space layout, where a trivial program builds all the same.)
VARIANTS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]}


def _compile(flags, src, exe):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", *flags,
                           "-I" + os.path.join(ROOT, "opencv_contrib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), src, "-o", exe],
                          capture_output=True, text=True)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_owners_host_semantics(tmp_path, variant):
    """tests/cpp/own_test.cpp, over a fake device whose events and blocks are malloc'd tokens, which knows every live one, logs its
    calls and fails the k-th call of a kind on request.
    Owned: ensure creates lazily and once; a failed create hands on the policy's code and leaves the owner empty and usable; release
    gives the handle up and the destructor then destroys nothing; a move leaves the source empty; a growing vector of owners destroys
    each handle exactly once.
    ArenaCache, with small limits passed in: a cached block serves bytes <= cap <= bytes + bytes / 2 + 64 MB, at both ends of the window
    and one past each; the smallest fitting block wins; a block of another device is never handed out; a miss allocates; a failing
    allocation trims and retries once, then MI_ERR_OOM with a text; a block is taken back at 4 blocks per device, at the per-device and
    the per-process byte bound and not one past any of them, not with a limit of 0 and not when the device cannot be synchronised; every
    event is destroyed exactly once on a hit, an eviction, a trim, a block not taken and a null block; a failed event wait on a hit
    clears the sticky error and synchronises the device, and where that fails too frees the block for a fresh one; a busy block without
    an event synchronises the BLOCK's device and restores the current one, as trimming does.
    CachedArena: mark without a block does nothing; under a capturing stream, with a failing event create and with a failing record it
    leaves used, no valid event, a cleared sticky error and no leak; release after a valid mark hands the event to the cache and keeps
    none; release is idempotent; acquire gives the held block back first; the destructor releases once.
    Last, three threads against one cache.  Plain C++, no device, its own process: once plain and once under
    -fsanitize=address,undefined (skipped only where a trivial program does not build with those flags)."""
    flags = VARIANTS[variant]
    if flags:
        trivial = tmp_path / "trivial.cpp"
        trivial.write_text("int main() { return 0; }\n")
        if _compile(flags, str(trivial), str(tmp_path / "trivial")).returncode != 0:
            pytest.skip("no address / undefined-behaviour sanitizer runtime for g++ on this machine")
    exe = str(tmp_path / "own_test")
    r = _compile(flags, os.path.join(ROOT, "tests", "cpp", "own_test.cpp"), exe)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "own_test: ok" in r.stdout, r.stdout + r.stderr
