"""What the sanitizer tests share: a stand-alone driver program (tests/host/*.c) linked with the library's host sources -- every
csrc/*.cpp, and agx_text.c -- compiled under the sanitizers, and with its device objects unchanged; the program runs on the CPU
build and touches no device.  Nothing is loaded into Python under a sanitizer."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "accelerating-genomics_amd")
CLANG = "/opt/rocm/lib/llvm/bin/clang"

ASAN_UBSAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def run_driver(tmp_path, driver, ok_token, needs_object, sanitizers="address,undefined", defines=(), args=(), env_extra=ASAN_UBSAN_ENV):
    """Builds tests/host/<driver>.c against the sanitized host sources and runs it: exit status 0, ok_token on stdout, no
    sanitizer report on stderr.  needs_object: the device object whose absence means the library has not been built yet."""
    import accelerating_genomics_amd.api as agx

    if not os.path.exists(os.path.join(PKG, "build", needs_object)):
        agx.build()
    san = ["-fsanitize=" + sanitizers, "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", *defines]
    objs = []
    for src in sorted(glob.glob(os.path.join(PKG, "csrc", "*.cpp"))):
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([CLANG + "++", "-std=c++17", "-x", "c++", *san, *inc, "-c", src, "-o", o], check=True)
        objs.append(o)
    for src, extra in ((os.path.join(PKG, "csrc", "agx_text.c"), ["-D_POSIX_C_SOURCE=200809L"]),
                       (os.path.join(ROOT, "tests", "host", driver + ".c"), [])):
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([CLANG, "-std=c99", *san, *inc, *extra, "-c", src, "-o", o], check=True)
        objs.append(o)
    dev = sorted(glob.glob(os.path.join(PKG, "build", "agx_*_kernel.o")))  # every device object, linked unchanged
    exe = str(tmp_path / driver)
    subprocess.run([CLANG + "++", *san, *objs, *dev, "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe, *args], capture_output=True, env=dict(os.environ, **env_extra), timeout=600)
    tail = (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    assert r.returncode == 0 and ok_token in r.stdout, tail
    assert b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, tail
