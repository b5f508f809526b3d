"""Static half of the stream contract (include/mmf_hg.h: "Every call enqueues on `hip_stream`"): a scan of the host code in
multimodal-fusion_amd/csrc.  tests/test_gpu_stream_contract.py runs every entry behind a closed gate on a side stream, but
cannot reach every rare branch; this test reads every launch and every runtime call instead.

  * every kernel launch and every asynchronous runtime call names a stream that is not the null stream;
  * every BLOCKING copy, memset or device synchronisation sits in a function that is listed below with its reason.

It also checks that the table of INTEGRATION.md ("Host synchronisations and host arguments") and the SYNC dictionary of the
GPU test list the same entries with the same words."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal-fusion_amd", "csrc")

NULL_STREAMS = {"0", "NULL", "nullptr", "(hipStream_t)0", "(hipStream_t)NULL", "(hipStream_t)nullptr", "hipStreamDefault",
                "hipStreamLegacy", "hipStreamPerThread"}

# (file, enclosing function) -> why a blocking call is in order there
BLOCKING_ALLOWED = {
    ("mmf_api.hip", "run"): "after the call's hipStreamSynchronize: the MMF_SYMMETRIC_DEBUG dump and the fail-row diagnostics "
                                     "of an error message read a few words the stream has already written",
    ("mmf_api.hip", "mmf_simtopk_segmented"): "the flagged rows are read back right after the call's hipStreamSynchronize(s)",
    ("mmf_api.hip", "mmf_release_workspaces"): "frees every cached workspace: the device must be idle first, whatever the stream",
    ("mmf_order.hip", "query_order_last"): "diagnostics entry without a stream (mmf_debug_query_order): reads the recorded permutation",
}

# asynchronous runtime calls and where their stream argument is (counted from the end for the copies and memsets)
STREAM_LAST = re.compile(r"\b(hip(?:Memcpy|Memset|Malloc|Free|MemPrefetch)\w*Async)\s*\(")
HIPCUB = re.compile(r"\b(hipcub::\w+::\w+)\s*\(")
LAUNCH = re.compile(r"\bhipLaunchKernelGGL\s*\(")
CHEVRON = re.compile(r"<<<")
STREAM_AT = {"hipEventRecord": 1, "hipStreamWaitEvent": 0, "hipLaunchKernel": 5, "hipLaunchCooperativeKernel": 5,
             "hipModuleLaunchKernel": 8, "hipExtLaunchKernelGGL": 4}
BLOCKING = re.compile(r"\b(hipMemcpy\w*|hipMemset\w*|hipDeviceSynchronize)\s*\(")
FUNCTION = re.compile(r"^(?![ \t#/}])[^;{}()]*?\b([A-Za-z_]\w*)\s*\((?:[^;{}()]|\([^()]*\))*\)\s*(?:const\s*)?\{", re.M)


def sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, strip_comments(f.read())


def strip_comments(text):
    """Comments and string literals blanked, line structure kept."""
    def blank(m):
        return re.sub(r"[^\n]", " ", m.group(0))
    return re.sub(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"", blank, text, flags=re.S)


def call_args(text, open_paren):
    """The top-level arguments of the call whose '(' is at text[open_paren]."""
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(text)):
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(text[start:i])
                return [re.sub(r"\s+", " ", a).strip() for a in args]
        elif c == "," and depth == 1:
            args.append(text[start:i])
            start = i + 1
    raise AssertionError("unbalanced call")


def line_of(text, pos):
    return text.count("\n", 0, pos) + 1


def is_null(arg):
    return arg.replace(" ", "") in {s.replace(" ", "") for s in NULL_STREAMS}


def enclosing(text, pos):
    name = None
    for m in FUNCTION.finditer(text):
        if m.start() > pos:
            break
        name = m.group(1)
    return name


def stream_uses():
    """(file, line, what, stream expression, all arguments) of every launch and asynchronous runtime call."""
    for name, text in sources():
        for m in LAUNCH.finditer(text):
            a = call_args(text, m.end() - 1)
            assert len(a) >= 5, f"{name}:{line_of(text, m.start())}: hipLaunchKernelGGL with {len(a)} arguments"
            yield name, line_of(text, m.start()), "hipLaunchKernelGGL", a[4], a
        for m in CHEVRON.finditer(text):
            end = text.index(">>>", m.end())
            a = call_args("(" + text[m.end():end] + ")", 0)
            yield name, line_of(text, m.start()), "<<<>>>", a[3] if len(a) >= 4 else "0", a
        for m in STREAM_LAST.finditer(text):
            a = call_args(text, m.end() - 1)
            yield name, line_of(text, m.start()), m.group(1), a[-1], a
        for m in HIPCUB.finditer(text):
            a = call_args(text, m.end() - 1)
            yield name, line_of(text, m.start()), m.group(1), a[-1], a
        for fn, at in STREAM_AT.items():
            for m in re.finditer(r"\b" + fn + r"\s*\(", text):
                a = call_args(text, m.end() - 1)
                yield name, line_of(text, m.start()), fn, a[at], a


def test_the_scanner_reads_calls_as_written():
    text = strip_comments('x = 1; // hipMemcpy(a, b)\nMMF_HIP(hipMemsetAsync(p, 0, (size_t)n * 4, s));\n'
                          'hipLaunchKernelGGL(k<A>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)0, f(a, b), c);\n')
    assert not BLOCKING.search(text.split("\n")[0])
    m = STREAM_LAST.search(text)
    assert call_args(text, m.end() - 1) == ["p", "0", "(size_t)n * 4", "s"]
    m = LAUNCH.search(text)
    a = call_args(text, m.end() - 1)
    assert a[4] == "(hipStream_t)0" and is_null(a[4]) and a[5] == "f(a, b)" and not is_null("s") and is_null("nullptr")
    src = "static int f(int a,\n         int b) {\n  g();\n}\nint h(void* p) { return 0; }\n"
    assert enclosing(src, src.index("g()")) == "f" and enclosing(src, src.index("return")) == "h"


def test_every_launch_and_async_call_names_the_callers_stream():
    uses = list(stream_uses())
    assert len(uses) > 150, len(uses)                  # the scan found the library (some 200 launches and runtime calls)
    size_queries, offenders = 0, []
    for name, line, what, stream, args in uses:
        if not is_null(stream):
            continue
        if what.startswith("hipcub::") and args[0] == "nullptr":
            size_queries += 1                           # the named exception: a size query (null temp storage) launches nothing
            continue
        offenders.append(f"{name}:{line}: {what} on the null stream ({stream})")
    assert not offenders, "\n".join(offenders)
    assert size_queries == 2


def test_blocking_calls_are_listed_with_their_reason():
    found, offenders = set(), []
    for name, text in sources():
        for m in BLOCKING.finditer(text):
            if m.group(1).endswith("Async"):
                continue
            where = (name, enclosing(text, m.start()))
            found.add(where)
            if where not in BLOCKING_ALLOWED:
                offenders.append(f"{name}:{line_of(text, m.start())}: blocking {m.group(1)} in {where[1]}()")
    assert not offenders, "\n".join(offenders)
    assert found == set(BLOCKING_ALLOWED), f"listed but no longer there: {sorted(set(BLOCKING_ALLOWED) - found)}"
    assert all(len(reason) > 20 for reason in BLOCKING_ALLOWED.values())


def integration_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.split(r"^## [0-9. ]*Host synchronisations and host arguments$", text, 1, flags=re.M)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = re.match(r"^\|\s*`(mmf_\w+)`\s*\|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|\s*$", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows


def test_integration_table_equals_the_gpu_tests_table():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_stream_contract import SYNC
    rows = integration_table()
    assert sorted(rows) == sorted(SYNC), sorted(set(rows) ^ set(SYNC))
    for entry, want in SYNC.items():
        assert rows[entry] == want, (entry, rows[entry], want)
    assert {s for s, _ in SYNC.values()} <= {"none", "once", "per iteration", "data-dependent"}
    with open(os.path.join(ROOT, "include", "mmf_hg.h")) as f:
        assert "Host synchronisations and host arguments" in f.read()          # the Conventions block points at the table
    # every exported entry that takes a stream is in the table (multimodal-fusion_amd/_lib.py EXPORTS)
    with open(os.path.join(ROOT, "multimodal-fusion_amd", "_lib.py")) as f:
        exports = set(re.findall(r"\"(mmf_\w+)\"", f.read().split("EXPORTS = [", 1)[1].split("]", 1)[0]))
    no_stream = {"mmf_version", "mmf_last_error", "mmf_padded_dim", "mmf_fast_scan_supported", "mmf_debug_query_order",
                 "mmf_debug_symmetric_schedule"}
    assert exports - no_stream == set(SYNC), sorted((exports - no_stream) ^ set(SYNC))
