"""`run_backtest.py backtest --portfolio` on the CPU path, and the engine
method behind it."""

import json
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent


def _cli(*args, data_dir):
    return subprocess.run(
        [sys.executable, str(REPO / "run_backtest.py"), "--data-dir",
         str(data_dir), *args],
        capture_output=True, text=True, timeout=300, cwd=REPO)


def test_cli_portfolio_cpu(tmp_path):
    d = tmp_path / "cli"
    r = _cli("backtest", "--portfolio", "AAAUSDC,BBBUSDC,CCCUSDC",
             "--max-positions", "2", "--strategy", "momentum", "--candles",
             "1500", "--cpu", data_dir=d)
    assert r.returncode == 0, r.stderr
    head, _, table = r.stdout.partition("\nsymbol ")
    stats = json.loads(head)
    assert stats["symbols"] == ["AAAUSDC", "BBBUSDC", "CCCUSDC"]
    assert stats["max_positions"] == 2 and stats["engine"] == "cpu"
    assert stats["n_candles"] == 1500
    for key in ("final_equity", "max_drawdown_pct", "sharpe", "n_trades",
                "refused_slots", "refused_cash"):
        assert key in stats
    rows = table.splitlines()
    assert rows[0].split() == ["trades", "win", "rate", "pnl"]
    assert [row.split()[0] for row in rows[1:5]] == [
        "AAAUSDC", "BBBUSDC", "CCCUSDC", "portfolio"]
    assert sum(int(row.split()[1]) for row in rows[1:4]) == stats["n_trades"]
    assert "entry signals untaken" in rows[4]

    r = _cli("list", data_dir=d)
    assert r.returncode == 0, r.stderr
    listed = json.loads(r.stdout)["results"]
    assert [x["symbol"] for x in listed] == [stats["symbol"]]
    assert listed[0]["n_trades"] == stats["n_trades"]


def test_cli_symbol_is_required_without_portfolio(tmp_path):
    r = _cli("backtest", "--cpu", data_dir=tmp_path)
    assert r.returncode == 2 and "--symbol" in r.stderr
    r = _cli("backtest", "--symbol", "AAAUSDC", "--max-positions", "2",
             "--cpu", data_dir=tmp_path)
    assert r.returncode == 2 and "--portfolio" in r.stderr
    r = _cli("backtest", "--portfolio", "AAAUSDC,BBBUSDC", "--max-positions",
             "3", "--cpu", "--candles", "300", data_dir=tmp_path)
    assert r.returncode != 0 and "max_positions" in r.stderr


def test_engine_portfolio_stats(tmp_path):
    from ai_crypto_trader_amd.backtesting.engine import BacktestEngine

    eng = BacktestEngine(str(tmp_path / "d"), device="cpu")
    symbols = ["AAAUSDC", "BBBUSDC", "CCCUSDC", "DDDUSDC"]
    stats = eng.run_portfolio_backtest(
        symbols, max_positions=2, strategy="momentum", n_candles=1500,
        equity_stride=10)
    assert stats["n_trades"] > 0
    assert len(stats["equity_curve"]) == 150
    assert stats["equity_curve"][-1] == pytest.approx(stats["final_equity"])
    assert [r["symbol"] for r in stats["per_symbol"]] == symbols
    assert sum(r["n_trades"] for r in stats["per_symbol"]) \
        == stats["n_trades"]
    assert eng.last_saved.exists()
    saved = json.loads(eng.last_saved.read_text())
    assert "equity_curve" not in saved and saved["symbols"] == symbols
    with pytest.raises(ValueError):
        eng.run_portfolio_backtest(symbols, max_positions=5)
    with pytest.raises(ValueError):
        eng.run_portfolio_backtest(symbols, max_positions=2, strategy="grid")
