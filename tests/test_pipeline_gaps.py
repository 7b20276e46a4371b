"""tools/pipeline_gaps.py on a hand-made kernel trace: the region cut, the encoder-idle time and the hidden share of every decoder
launch are what the intervals say."""
import os
import subprocess
import sys

from conftest import REPO

HEAD = '"Kind","Agent_Id","Queue_Id","Kernel_Name","Start_Timestamp","End_Timestamp"\n'


def _row(q, name, a, b):
    return f'"KERNEL_DISPATCH",0,{q},"{name}",{a},{b}\n'


def test_pipeline_gaps_on_a_synthetic_trace(tmp_path):
    ms = 1_000_000
    rows = [
        # warm-up: encoder on queue 1, decoder on queue 2
        _row(1, "attn_enc_dma_kernel<2>(AttnEncArgs)", 0, 1 * ms), _row(2, "head_rows_kernel(x)", 1 * ms, 2 * ms),
        # region: encoders on queues 1 and 3 from 10 ms to 20 ms with a hole 14-15 ms, then 22-30 ms on queue 1
        _row(3, "void gemm_pp2_kernel<0>(GemmArgs)", 10 * ms, 14 * ms), _row(1, "attn_enc_dma_kernel<2>(AttnEncArgs)", 12 * ms, 14 * ms),
        _row(3, "attn_enc_dma_kernel<2>(AttnEncArgs)", 15 * ms, 20 * ms), _row(1, "void gemm_pp2_kernel<0>(GemmArgs)", 22 * ms, 30 * ms),
        # decoder launch A on queue 2: 20-24 ms (half under the 22-30 encoder); B on queue 4: 30-32 ms (exposed)
        _row(2, "dec_cross_qk_kernel(DecQKArgs)", 20 * ms, 21 * ms), _row(2, "__amd_rocclr_copyBuffer", 19 * ms, 19 * ms + 5),
        _row(2, "head_rows_kernel(x)", 23 * ms, 24 * ms),
        _row(4, "dec_cross_qk_kernel(DecQKArgs)", 30 * ms, 31 * ms), _row(4, "head_rows_kernel(x)", 31 * ms, 32 * ms),
    ]
    f = tmp_path / "t_kernel_trace.csv"
    f.write_text(HEAD + "".join(rows))
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "pipeline_gaps.py"), str(f), "--launches", "2"],
                         capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    assert lines[0].startswith("timed region: 22.000 ms, 2 launch sequences, encoder queues ['1', '3']"), out
    assert lines[1].startswith("no encoder-class kernel running: 5.000 ms"), out          # 14-15, 20-22, 30-32
    assert "decoder launch 0 (queue 2): span 4.000 ms at +10.000 ms,  50.0 % under encoder kernels" in lines[2], out
    assert "decoder launch 1 (queue 4): span 2.000 ms at +20.000 ms,   0.0 % under encoder kernels" in lines[3], out
    assert lines[4].startswith("decoder spans in all: 6.000 ms, 33.3 % under encoder kernels, 4.000 ms exposed"), out
    bad = subprocess.run([sys.executable, os.path.join(REPO, "tools", "pipeline_gaps.py"), str(f), "--launches", "3"], capture_output=True, text=True)
    assert bad.returncode != 0 and "nothing to cut" in bad.stderr
