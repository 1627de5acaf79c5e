"""Repo-convention meta tests (reference: test_no_emoji_in_source.py,
test_file_header_convention.py, test_config_centralization.py,
test_sql_injection_params.py)."""

import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "audiomuse_amd")

_EMOJI = re.compile("[\U0001F300-\U0001FAFF\U00002600-\U000027BF]")

# modules allowed to read the environment directly (everything else goes
# through audiomuse_amd.config)
_ENV_ALLOWED = {
    os.path.join("audiomuse_amd", "config.py"),
    os.path.join("audiomuse_amd", "web", "auth.py"),      # admin seed env
    os.path.join("audiomuse_amd", "web", "api_chat.py"),  # AI provider creds
    os.path.join("audiomuse_amd", "parallel", "dist.py"), # torchrun env
    os.path.join("audiomuse_amd", "__main__.py"),
    # passes the process env through to spawned worker subprocesses
    # (HIP_VISIBLE_DEVICES pinning) — not a config read
    os.path.join("audiomuse_amd", "standalone.py"),
}


def _py_files():
    for base, _dirs, files in os.walk(PKG):
        if "__pycache__" in base:
            continue
        for f in files:
            if f.endswith(".py"):
                yield os.path.join(base, f)


def test_no_emoji_in_source():
    for path in _py_files():
        with open(path, encoding="utf-8") as fh:
            text = fh.read()
        assert not _EMOJI.search(text), f"emoji in {path}"


def test_module_docstrings():
    import ast

    missing = []
    for path in _py_files():
        if os.path.basename(path) == "__init__.py" and \
                os.path.getsize(path) < 200:
            continue
        with open(path, encoding="utf-8") as fh:
            tree = ast.parse(fh.read())
        if ast.get_docstring(tree) is None:
            missing.append(os.path.relpath(path, ROOT))
    assert not missing, f"modules without docstrings: {missing}"


def test_env_reads_centralized():
    offenders = []
    for path in _py_files():
        rel = os.path.relpath(path, ROOT)
        if rel in _ENV_ALLOWED:
            continue
        with open(path, encoding="utf-8") as fh:
            text = fh.read()
        if "os.environ" in text or "os.getenv" in text:
            offenders.append(rel)
    assert not offenders, f"env reads outside config: {offenders}"


def test_sql_injection_safe(tmp_path):
    """Hostile strings through the query endpoints never reach SQL
    unparameterized (reference: test_sql_injection_params.py)."""
    from audiomuse_amd.db import connect
    from audiomuse_amd.db.schema import init_db
    from audiomuse_amd.db.store import save_track_analysis_and_embedding
    from audiomuse_amd.web.app import create_app

    url = f"sqlite:///{tmp_path}/inj.db"
    conn = connect(url)
    init_db(conn)
    rng = np.random.default_rng(0)
    save_track_analysis_and_embedding(
        conn, "fp_4" + "0" * 50, title="Safe", author="A",
        embedding=rng.standard_normal(200).astype(np.float32))
    app = create_app(url, auth_disabled=True)
    app.testing = True
    evil = "'; DROP TABLE score;--"
    with app.test_client() as client:
        r = client.get(f"/api/search_tracks?q={evil}")
        assert r.status_code == 200 and r.json == []
        r = client.get(f"/api/similar_tracks?item_id={evil}")
        assert r.status_code in (404, 503)
        client.post("/chat/api/chatPlaylist", json={"prompt": evil})
    # table survived
    assert conn.execute("SELECT COUNT(*) FROM score").fetchone()[0] == 1
    conn.close()


def test_no_cuda_or_hipify_artifacts():
    """No CUDA shims / hipify output / multi-backend dispatch in the
    native sources (north-star constraint)."""
    csrc = os.path.join(PKG, "ops", "csrc")
    for f in os.listdir(csrc):
        with open(os.path.join(csrc, f), encoding="utf-8") as fh:
            text = fh.read()
        assert "cudaMalloc" not in text and "cuda_runtime" not in text, f
        assert "__CUDA_ARCH__" not in text, f


def test_config_surface_and_centralization():
    """Reference analog: test_config_centralization.py — the config
    module is the single source of tunables: every documented parameter
    exists, the surface stays at reference scale (>=250 settings), and
    PARAMETERS.md stays in sync with the module."""
    import re

    import audiomuse_amd.config as C

    names = [k for k in dir(C) if k.isupper() and not k.startswith("_")]
    assert len(names) >= 250, f"config surface shrank: {len(names)}"

    doc = open(os.path.join(ROOT, "docs", "PARAMETERS.md")).read()
    documented = set(re.findall(r"\| `([A-Z][A-Z0-9_]*)` \|", doc))
    missing = documented - set(names)
    assert not missing, f"PARAMETERS.md documents unknown settings: {missing}"
    undocumented = set(names) - documented
    assert not undocumented, \
        f"settings missing from docs/PARAMETERS.md: {undocumented}"


def test_config_settings_are_consumed():
    """Each group of settings must have real consumers — a config
    surface of dead names is padding, not parity. Spot-checks one
    representative knob per subsystem by grepping the package source."""
    import subprocess

    pkg = os.path.join(ROOT, "audiomuse_amd")
    for rep in ["DBSCAN_EPS_MIN", "SCORE_WEIGHT_DIVERSITY",
                "IVF_RESULT_CACHE_SECONDS", "CHROMAPRINT_ALIGN_RANGE",
                "MEDIASERVER_RETRIES", "MUSIC_LIBRARIES",
                "WHISPER_REPETITION_PENALTY", "AI_TOOLCALL_TEMPERATURE",
                "PLUGIN_MAX_DOWNLOAD_MB", "CLEANING_SAFETY_LIMIT",
                "SWEEP_PRUNE_MIN_FETCH_RATIO", "ALCHEMY_TEMPERATURE",
                "PATH_DEFAULT_LENGTH", "SONIC_FINGERPRINT_TOP_PLAYED",
                "EXPLOITATION_START_FRACTION", "OLLAMA_SERVER_URL",
                "SIMILARITY_ELIMINATE_DUPLICATES_DEFAULT",
                "POSTGRES_HOST", "IVF_KMEANS_BATCH", "TOP_N_ELITES"]:
        hits = subprocess.run(
            # source files only: a byte-compiled config module under
            # __pycache__ also holds every name and is no consumer
            ["grep", "-rl", "--include=*.py", rep, pkg],
            capture_output=True, text=True
        ).stdout.strip().splitlines()
        consumers = [h for h in hits if not h.endswith("config.py")]
        assert consumers, f"config setting {rep} has no consumer"
