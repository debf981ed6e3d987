"""CPU: the generator has no shared state -- two threads generating the sources of two different systems get, every time, the text
each gets alone, and ThreadSanitizer sees no race.  A stand-alone program (tests/cpp/codegen_threads.cpp, its own main) compiled with
hamilton_amd/csrc/hamk_codegen.cpp under -fsanitize=thread and run as a child process; nothing is loaded into this one.
(file-scope emit state, read by emit_body and written by generate_source, under handles that build lazily and concurrently.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_threads_generate_what_each_generates_alone(tmp_path):
    exe = str(tmp_path / "codegen_threads")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hamilton_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "codegen_threads.cpp"),
                           os.path.join(ROOT, "hamilton_amd", "csrc", "hamk_codegen.cpp"), "-o", exe])
    env = dict(os.environ, TSAN_OPTIONS="exitcode=66 halt_on_error=0")
    r = subprocess.run([exe, "10"], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert "ThreadSanitizer" not in r.stderr, "ThreadSanitizer reported:\n" + r.stderr[:4000]
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "0 differ; lane" in r.stdout and r.stdout.rstrip().endswith(", 0 differ")
