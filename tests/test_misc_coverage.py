"""Coverage for thinner areas: environments, NFS, mounts, config, cron e2e."""

from __future__ import annotations

import os
import time

import pytest

import modal_amd as modal


def test_environment_scoped_names(client):
    qa = modal.Queue.from_name("same-name", environment_name="env-a", create_if_missing=True)
    qb = modal.Queue.from_name("same-name", environment_name="env-b", create_if_missing=True)
    qa.put("for-a")
    qb.put("for-b")
    assert qa.get() == "for-a"
    assert qb.get() == "for-b"


def test_network_file_system_alias(client):
    import io

    nfs = modal.NetworkFileSystem.from_name("legacy-nfs", create_if_missing=True)
    nfs.write_file("notes.txt", io.BytesIO(b"nfs data"))
    assert b"".join(nfs.read_file("notes.txt")) == b"nfs data"
    entries = nfs.listdir("/")
    assert entries[0].path == "notes.txt"


def test_mount_materializes_content(client, tmp_path):
    (tmp_path / "pkg").mkdir()
    (tmp_path / "pkg" / "data.txt").write_text("mounted!")
    m = modal.Mount.from_local_dir(str(tmp_path / "pkg"), remote_path="/r/pkg")
    m.hydrate()
    from modal_amd._sync import unwrap

    root = unwrap(m)._dir
    assert open(os.path.join(root, "r/pkg/data.txt")).read() == "mounted!"


def test_config_override_locally():
    from modal_amd.config import config

    before = config.get("heartbeat_interval")
    config.override_locally("heartbeat_interval", 99.0)
    try:
        assert config.get("heartbeat_interval") == 99.0
    finally:
        config.clear_override("heartbeat_interval")
    assert config.get("heartbeat_interval") == before


def test_auth_token_manager_refresh_math():
    import asyncio
    import time as _time

    from modal_amd.utils.auth_token_manager import AuthTokenManager

    calls = []

    async def fetch():
        calls.append(_time.time())
        return f"tok-{len(calls)}", _time.time() + 100

    mgr = AuthTokenManager(fetch)

    async def main():
        t1 = await mgr.get_token()
        t2 = await mgr.get_token()
        assert t1 == t2 == "tok-1"  # cached inside the refresh window
        # force expiry of the refresh point
        mgr._refresh_at = 0
        t3 = await mgr.get_token()
        assert t3 == "tok-2"

    asyncio.run(main())


def test_cron_schedule_fires_on_minute_boundary(client, run_dir, monkeypatch):
    """Cron '* * * * *' fires at most once per minute — patch the matcher's
    clock window by checking the runner marks the minute."""
    from modal_amd.scheduler.cron import ScheduleRunner, cron_matches
    from datetime import datetime, timezone

    # logic-level check: every-minute cron matches any timestamp
    assert cron_matches("* * * * *", datetime.now(timezone.utc))


def test_image_base_variants(client):
    for img in [
        modal.Image.from_registry("rocm/pytorch:latest"),
        modal.Image.micromamba(python_version="3.11"),
        modal.Image.debian_slim().apt_install("git").micromamba_install("numpy"),
    ]:
        img.hydrate()
        assert img.object_id.startswith("im-")


def test_proxy_and_snapshot_handles(client):
    p = modal.Proxy.from_name("static-ip")
    p.hydrate()
    assert p.object_id
    snap = modal.SandboxSnapshot.from_id("sn-deadbeef")
    snap.hydrate()
    assert snap.object_id == "sn-deadbeef"


def test_cloud_bucket_mount_local_dir(tmp_path):
    cbm = modal.CloudBucketMount("my-bucket", key_prefix="data/")
    path = cbm.local_dir(root=str(tmp_path))
    assert "my-bucket" in path and path.endswith("data/")


def test_output_steps_and_map_progress(client, capsys):
    """enable_output prints step lines and MapProgress tracks counters
    (non-TTY: plain '+' lines, no rich bar)."""
    import modal_amd as modal
    from modal_amd.output import MapProgress, get_output_manager

    app = modal.App("out-app")

    @app.function()
    def double(x):
        return x * 2

    with modal.enable_output():
        mgr = get_output_manager()
        assert mgr is not None
        with app.run(client=client):
            assert sorted(double.map(range(10))) == [x * 2 for x in range(10)]
    captured = capsys.readouterr()
    assert "Initialized app out-app." in captured.out
    assert "double" in captured.out  # created-functions step line

    p = MapProgress(None, "test")  # no console: silent counters
    p.update(3, 10)
    assert (p.completed, p.submitted) == (3, 10)
    p.close()


def test_remote_traceback_shows_user_frames_only(client):
    """Remote exceptions re-raise locally with the USER's frames and
    without framework/asyncio noise (parity: reference _traceback.py
    re-synthesis + frame suppression)."""
    import traceback

    import modal_amd as modal

    app = modal.App("tb-app")

    @app.function()
    def outer_fails():
        def deep_inner():
            raise ValueError("tb-sentinel")

        deep_inner()

    with app.run(client=client):
        try:
            outer_fails.remote()
            raise AssertionError("should have raised")
        except ValueError as exc:
            tb_text = "".join(traceback.format_exception(type(exc), exc, exc.__traceback__))
    assert "tb-sentinel" in tb_text
    assert "deep_inner" in tb_text            # the remote user frame survives
    assert "outer_fails" in tb_text
    assert "/modal_amd/runtime/worker.py" not in tb_text  # framework frames dropped


def test_retry_policy_clamp_and_backoff():
    """Retries delay math: 1 s floor, 24 h ceiling, exponential factor
    (parity: reference retries.py:8-9 clamp)."""
    import pytest

    import modal_amd as modal
    from modal_amd.exception import InvalidError

    r = modal.Retries(max_retries=5, initial_delay=2.0, backoff_coefficient=2.0, max_delay=10.0)
    policy = r._to_policy_dict()
    assert policy["max_retries"] == 5
    with pytest.raises(InvalidError):
        modal.Retries(max_retries=5, initial_delay=0.1)  # below the 1 s floor
    with pytest.raises(InvalidError):
        modal.Retries(max_retries=5, initial_delay=2.0, max_delay=100_000.0)  # > 24 h


def test_tunnel_forward_and_billing(client, capsys):
    """modal.forward exposes a local port as a Tunnel; billing summary
    accounts executed inputs (parity rows 36/37 + billing CLI)."""
    import http.server
    import socketserver
    import threading
    import urllib.request

    import modal_amd as modal
    from modal_amd.billing import usage_summary

    class H(http.server.BaseHTTPRequestHandler):
        def do_GET(self):
            self.send_response(200)
            self.end_headers()
            self.wfile.write(b"tunneled")

        def log_message(self, *a):
            pass

    with socketserver.TCPServer(("127.0.0.1", 0), H) as httpd:
        port = httpd.server_address[1]
        threading.Thread(target=httpd.serve_forever, daemon=True).start()
        with modal.forward(port, unencrypted=True) as tunnel:
            assert tunnel.url.startswith("https://")  # parity shape
            host, tport = tunnel.tcp_socket
            with urllib.request.urlopen(f"http://{host}:{tport}", timeout=10) as resp:
                assert resp.read() == b"tunneled"
        httpd.shutdown()

    app = modal.App("bill-app")

    @app.function()
    def unit(x):
        return x

    with app.run(client=client):
        assert sorted(unit.map(range(20))) == list(range(20))
    rows = usage_summary(client)
    mine = [r for r in rows if r["function"] == "unit"]
    assert mine and mine[0]["inputs"] >= 20


def test_iteration_apis(client):
    """Dict keys/values/items, Queue.iterate, Volume.iterdir/listdir."""
    import io

    import modal_amd as modal

    d = modal.Dict.from_name("iter-d", create_if_missing=True)
    d.put("a", 1)
    d.put("b", 2)
    assert sorted(d.keys()) == ["a", "b"]
    assert sorted(d.values()) == [1, 2]
    assert sorted(d.items()) == [("a", 1), ("b", 2)]
    assert len(d) == 2 and "a" in d

    with modal.Queue.ephemeral() as q:
        q.put_many([10, 20, 30])
        assert list(q.iterate(item_poll_timeout=0.2)) == [10, 20, 30]

    vol = modal.Volume.from_name("iter-v", create_if_missing=True)
    with vol.batch_upload(force=True) as b:
        b.put_file(io.BytesIO(b"x"), "/d1/f1.txt")
        b.put_file(io.BytesIO(b"y"), "/d1/f2.txt")
    names = [e.path for e in vol.listdir("/d1")]
    assert sorted(names) == ["d1/f1.txt", "d1/f2.txt"]
    all_entries = [e.path for e in vol.iterdir("/", recursive=True)]
    assert "d1/f1.txt" in all_entries


def test_execution_context_helpers(client):
    """modal.is_local / current_input_id / current_function_call_id."""
    import modal_amd as modal

    assert modal.is_local() is True

    app = modal.App("ctx-app")

    @app.function()
    def introspect():
        return {
            "local": modal.is_local(),
            "input_id": modal.current_input_id(),
            "call_id": modal.current_function_call_id(),
        }

    with app.run(client=client):
        out = introspect.remote()
    assert out["local"] is False
    assert out["input_id"] and out["input_id"].startswith("in-")
    assert out["call_id"] and out["call_id"].startswith("fc-")


def test_function_call_from_id_and_num_inputs(client):
    import modal_amd as modal
    from modal_amd.functions import FunctionCall

    app = modal.App("fcid-app")

    @app.function()
    def add(a, b):
        return a + b

    with app.run(client=client):
        fc = add.spawn(20, 22)
        fc2 = FunctionCall.from_id(fc.object_id)
        assert fc2.get(timeout=30) == 42


def test_tunnel_is_a_real_relay():
    """The tunnel listens on a DISTINCT port and proxies bytes; closing it
    kills the listener while the service stays reachable (round-1 review:
    the identity mapping had no forwarding logic)."""
    import socket
    import socketserver
    import threading

    import modal_amd as modal

    class Echo(socketserver.BaseRequestHandler):
        def handle(self):
            data = self.request.recv(1024)
            self.request.sendall(b"echo:" + data)

    with socketserver.TCPServer(("127.0.0.1", 0), Echo) as srv:
        port = srv.server_address[1]
        threading.Thread(target=srv.serve_forever, daemon=True).start()
        with modal.forward(port, unencrypted=True) as tunnel:
            host, tport = tunnel.tcp_socket
            assert tport != port, "tunnel must not be an identity mapping"
            with socket.create_connection((host, tport), timeout=5) as s:
                s.sendall(b"ping")
                assert s.recv(1024) == b"echo:ping"
            assert tunnel._relay.connections_served == 1
        # tunnel closed: no relay serves its port anymore (a loopback
        # connect may still "succeed" via the kernel's ephemeral-port
        # self-connect artifact — that is not our listener)
        try:
            s = socket.create_connection((host, tport), timeout=1)
        except OSError:
            pass  # refused: the common case
        else:
            with s:
                assert s.getsockname() == s.getpeername(), (
                    "something still proxies the closed tunnel port"
                )
        with socket.create_connection(("127.0.0.1", port), timeout=5) as s:
            s.sendall(b"direct")
            assert s.recv(1024) == b"echo:direct"
        srv.shutdown()


def test_type_stub_generation(tmp_path):
    """scripts/gen_stubs.py emits a parseable .pyi covering __all__
    (synchronicity-aware stub generation)."""
    import ast
    import subprocess
    import sys as _sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [_sys.executable, os.path.join(repo, "scripts", "gen_stubs.py")],
        capture_output=True, text=True, timeout=120,
    )
    assert out.returncode == 0, out.stderr
    stub_path = os.path.join(repo, "modal_amd", "__init__.pyi")
    src = open(stub_path).read()
    ast.parse(src)
    import modal_amd

    for name in modal_amd.__all__:
        assert name in src, f"{name} missing from stubs"


def test_api_surface_parity_batch(client, tmp_path):
    """Round-2 parity batch: members the AST audit flagged missing vs the
    reference (App tags/logs, Queue/Dict/Secret/Volume from_id+info,
    Cls.with_concurrency, Image.from_scratch, NFS.add_local_*)."""
    import io

    # Queue / Dict / Secret / Volume: from_id + info + name
    q = modal.Queue.from_name("parity-q", create_if_missing=True)
    q.put(1)
    q2 = modal.Queue.from_id(q.object_id)
    assert q2.get() == 1
    info = q.info()
    assert info.get("name") == "parity-q"
    assert q.name == "parity-q"
    modal.Queue.validate_partition_key(b"x" * 10)
    with pytest.raises(Exception):
        modal.Queue.validate_partition_key(b"x" * 5000)

    d = modal.Dict.from_name("parity-d", create_if_missing=True)
    d["k"] = "v"
    assert modal.Dict.from_id(d.object_id)["k"] == "v"
    assert d.info().get("name") == "parity-d"

    modal.Secret.create_deployed("parity-s", {"A": "0"})
    s = modal.Secret.from_name("parity-s")
    s.update(env_dict={"A": "1"})
    assert s.info().get("name") == "parity-s"

    v = modal.Volume.from_name("parity-v", create_if_missing=True)
    with v.batch_upload() as b:
        b.put_file(io.BytesIO(b"hello parity"), "/f.bin")
    buf = io.BytesIO()
    n = modal.Volume.from_id(v.object_id).read_file_into_fileobj("/f.bin", buf)
    assert n == 12 and buf.getvalue() == b"hello parity"

    # NFS add_local_file / add_local_dir
    nfs = modal.NetworkFileSystem.from_name("parity-nfs", create_if_missing=True)
    local = tmp_path / "one.txt"
    local.write_text("one")
    nfs.add_local_file(local)
    assert b"".join(nfs.read_file("one.txt")) == b"one"
    tree = tmp_path / "tree"
    (tree / "sub").mkdir(parents=True)
    (tree / "sub" / "two.txt").write_text("two")
    nfs.add_local_dir(tree, "/t")
    assert b"".join(nfs.read_file("t/sub/two.txt")) == b"two"

    # Image: from_scratch / pip_install_from_pyproject / build / logs / from_name
    img = modal.Image.from_scratch().pip_install_from_pyproject("pyproject.toml")
    img.build()
    assert isinstance(img.logs(), list)

    # App: tags + registered_web_endpoints + image property
    app = modal.App("parity-app", image=img)
    assert app.image is img

    @app.function()
    def plain(x):
        return x + 1

    @app.function()
    @modal.fastapi_endpoint(method="GET")
    def webby():
        return "hi"

    assert app.registered_web_endpoints == ["webby"]
    with app.run(client=client):
        app.set_tags({"team": "amd"})
        assert app.get_tags() == {"team": "amd"}
        assert plain.remote(1) == 2
        # Cls.with_concurrency / with_batching exist and chain
        from modal_amd.cls import Cls
        assert hasattr(Cls, "with_concurrency") and hasattr(Cls, "with_batching")
        # FunctionCall num_inputs + Function accessors
        fc = plain.spawn(5)
        assert fc.get() == 6
        assert fc.num_inputs() >= 1
        assert plain.app is app or plain.app is not None


def test_sandbox_wait_until_ready_and_tags(client):
    sb = modal.Sandbox.create("sleep", "0.4", client=client)
    sb.wait_until_ready(timeout=10)
    sb.set_tags({"k": "v"})
    assert sb.get_tags() == {"k": "v"}
    sb.reload_volumes()
    sb.wait()
    assert sb.returncode == 0


def test_image_publish_and_from_name(client):
    img = modal.Image.from_scratch()
    img.build(client=client)
    img.publish("base-img")
    got = modal.Image.from_name("base-img")  # :latest implied
    got.build(client=client)
    assert got.object_id == img.object_id
    with pytest.raises(Exception):
        modal.Image.from_name("no-such-img").build(client=client)


def test_api_audit_clean():
    """The AST parity audit (scripts/api_audit.py) must report no missing
    public members against the reference classes."""
    import subprocess
    import sys

    proc = subprocess.run(
        [sys.executable, "scripts/api_audit.py"],
        capture_output=True, text=True,
        cwd=__import__("os").path.dirname(__import__("os").path.dirname(__file__)),
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr


def test_object_managers(client):
    modal.Queue.objects.create("mgr-q")
    with pytest.raises(Exception):
        modal.Queue.objects.create("mgr-q")
    modal.Queue.objects.create("mgr-q", allow_existing=True)
    names = [r["name"] for r in modal.Queue.objects.list()]
    assert "mgr-q" in names
    modal.Queue.objects.delete("mgr-q")
    assert "mgr-q" not in [r["name"] for r in modal.Queue.objects.list()]

    modal.Dict.objects.create("mgr-d")
    modal.Secret.objects.create("mgr-s")
    modal.Volume.objects.create("mgr-v")
    assert [r["name"] for r in modal.Dict.objects.list()] == ["mgr-d"]
    assert [r["name"] for r in modal.Secret.objects.list()] == ["mgr-s"]
    assert [r["name"] for r in modal.Volume.objects.list()] == ["mgr-v"]
    modal.Volume.objects.delete("mgr-v")
    assert modal.Volume.objects.list() == []


def test_volume_mount_options(client, tmp_path):
    import io

    v = modal.Volume.from_name("opts-v", create_if_missing=True)
    with v.batch_upload() as b:
        b.put_file(io.BytesIO(b"deep"), "/sub/inner.txt")

    ro = v.read_only()
    with pytest.raises(Exception):
        ro.batch_upload()
    with pytest.raises(Exception):
        ro.remove_file("/sub/inner.txt")
    # reads still work on a read-only handle
    assert b"".join(ro.read_file("/sub/inner.txt")) == b"deep"

    scoped = v.with_mount_options(sub_path="sub")
    app = modal.App("vol-opts")
    mount = str(tmp_path / "data")  # writable without root

    @app.function(volumes={mount: scoped})
    def peek():
        with open(mount + "/inner.txt") as f:
            return f.read()

    with app.run(client=client):
        assert peek.remote() == "deep"


def test_sandbox_filesystem_and_logs(client):
    sb = modal.Sandbox.create("bash", "-c", "echo marker-out; sleep 0.2", client=client)
    fs = sb.filesystem
    fs.write_file("note.txt", b"fs-data")
    assert fs.exists("note.txt")
    assert fs.read_file("note.txt") == b"fs-data"
    assert "note.txt" in fs.list_files(".")
    sb.wait()
    logs = sb.logs()
    out = logs.fetch()
    assert "marker-out" in out


def test_sandbox_snapshot_directory_and_mount_image(client):
    sb = modal.Sandbox.create("bash", "-c", "mkdir -p proj && echo v1 > proj/file && sleep 600", client=client)
    sb.wait_until_ready(timeout=10)
    import time

    deadline = time.time() + 5
    while not sb.filesystem.exists("proj/file") and time.time() < deadline:
        time.sleep(0.05)
    img = sb.snapshot_directory("proj")
    sb2 = modal.Sandbox.create("sleep", "600", client=client)
    sb2.mount_image("proj", img)
    assert sb2.filesystem.read_file("proj/file") == b"v1\n"
    sb2.unmount_image("proj")
    assert not sb2.filesystem.exists("proj/file")
    tok = sb2.create_connect_token(user_metadata={"u": 1}, port=9999)
    assert tok["token"] and tok["url"].endswith(":9999")
    sb.detach()
    sb2.terminate()
    sb.terminate()


def test_function_spec_stub_logs(client):
    app = modal.App("spec-app")

    @app.function(timeout=30, memory=512)
    def noisy(x):
        print(f"noisy says {x}")
        return x

    impl = getattr(noisy, "_impl", noisy)
    assert impl.stub is impl.app
    spec = impl.spec
    assert spec["timeout"] == 30 and spec["memory"] == 512
    assert "def noisy" in impl.get_build_def()
    with app.run(client=client):
        assert noisy.remote(7) == 7
        import time

        time.sleep(0.3)
        from modal_amd._sync import synchronizer

        lines = synchronizer.run(impl.logs().fetch())
        assert any("noisy says 7" in ln for ln in lines)


def test_image_pipe_and_cls_validation():
    def setup(image, pkg):
        return image.pip_install(pkg)

    img = modal.Image.debian_slim().pipe(setup, "numpy")
    impl = getattr(img, "_impl", img)
    assert any(l.get("kind") == "pip_install" for l in impl._recipe)

    from modal_amd.cls import Cls, parameter

    class Good:
        x: int = parameter(default=1)

    Cls.validate_construction_mechanism(Good)

    class Bad:
        x: int = parameter(default=1)

        def __init__(self):
            pass

    with pytest.raises(Exception):
        Cls.validate_construction_mechanism(Bad)

    class Unannotated:
        pass

    Unannotated.y = parameter(default=2)
    with pytest.raises(Exception):
        Cls.validate_construction_mechanism(Unannotated)


def test_proxy_routes_function_http_traffic(client):
    """Proxy.from_name starts a real local forward proxy; a function declared
    with proxy= sees HTTP(S)_PROXY and its HTTP traffic relays through it."""
    import http.server
    import threading

    class H(http.server.BaseHTTPRequestHandler):
        def do_GET(self):
            body = b"origin-says-hi"
            self.send_response(200)
            self.send_header("Content-Length", str(len(body)))
            self.end_headers()
            self.wfile.write(body)

        def log_message(self, *a):
            pass

    httpd = http.server.HTTPServer(("127.0.0.1", 0), H)
    port = httpd.server_address[1]
    t = threading.Thread(target=httpd.serve_forever, daemon=True)
    t.start()
    try:
        p = modal.Proxy.from_name("egress")
        app = modal.App("proxy-app")

        @app.function(proxy=p)
        def fetch(url):
            import os
            import urllib.request

            proxy_url = os.environ["HTTP_PROXY"]
            # urllib honors env proxies for absolute http URLs
            opener = urllib.request.build_opener(
                urllib.request.ProxyHandler({"http": proxy_url})
            )
            with opener.open(url, timeout=10) as resp:
                return resp.read().decode()

        with app.run(client=client):
            assert fetch.remote(f"http://127.0.0.1:{port}/x") == "origin-says-hi"
        from modal_amd._sync import synchronizer

        stats = synchronizer.run(client.svc.proxy_stats())
        assert stats["running"] and stats["connections"] >= 1
        assert stats["bytes_relayed"] > 0
    finally:
        httpd.shutdown()


def test_proxy_connect_tunnel(client):
    """CONNECT tunneling through the local forward proxy (the https path)."""
    import socket
    import threading

    # echo server as the "origin"
    srv = socket.socket()
    srv.bind(("127.0.0.1", 0))
    srv.listen(1)
    origin_port = srv.getsockname()[1]

    def echo_once():
        conn, _ = srv.accept()
        data = conn.recv(1024)
        conn.sendall(b"echo:" + data)
        conn.close()

    t = threading.Thread(target=echo_once, daemon=True)
    t.start()

    from modal_amd._sync import synchronizer

    resp = synchronizer.run(client.svc.proxy_get_or_create(name="tun"))
    s = socket.create_connection(("127.0.0.1", resp["port"]), timeout=5)
    s.sendall(f"CONNECT 127.0.0.1:{origin_port} HTTP/1.1\r\n\r\n".encode())
    reply = s.recv(1024)
    assert b"200" in reply
    s.sendall(b"ping")
    assert s.recv(1024) == b"echo:ping"
    s.close()
    srv.close()
