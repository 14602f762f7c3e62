"""Phase cycles of the pph forward kernel at the EDSR body conv (diagnostics; needs a -DSR_BAND_STAMPS
build, SR_HIP_LIB).  Runs one conv (B 32, 64 x 64, 256 -> 256, residual operand) with the stamps on and
prints mean cycles per phase per block: wave 0's clocks at kernel entry, K loop start (end of the
prologue / of the re-stagger), K loop end, and the end of each half of the epilogue, per tile of the
block (clocks are compared within a block only: the XCDs' counters are not aligned).
usage: python tools/pph_stamps.py [variant [B [cin,cout,h]]]   (variant 80: the one-tile form)"""
import json
import sys

import torch

sys.path.insert(0, '.')
from basicsr4rs_amd.ops import conv as C  # noqa: E402


def main():
    variant = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    cin, cout, H = (int(v) for v in sys.argv[3].split(',')) if len(sys.argv) > 3 else (256, 256, 64)
    W = 64
    lib = C._lib.load()
    dt = torch.bfloat16
    torch.manual_seed(0)
    x = torch.randn(B, H, W, cin, device='cuda').to(dt)
    res = torch.randn(B, H, W, cout, device='cuda').to(dt)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1).cuda()
    wf, _, bg = C.prepared(conv.weight, conv.bias, C.ConvSpec(cin, cout), dt)
    y = torch.empty(B, H, W, cout, device='cuda', dtype=dt)
    nblk = 4096
    st = torch.zeros(nblk * 16, device='cuda', dtype=torch.int64)

    def run():
        C.conv_fwd_raw(x, wf, bg, y, B, H, W, cin, cout, cout, res=res, beta=1.0)

    C._lib.check(lib.sr_conv3x3_set_variant(variant))
    try:
        for _ in range(3):
            run()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(20):
            run()
        ev[1].record()
        torch.cuda.synchronize()
        us = ev[0].elapsed_time(ev[1]) * 1e3 / 20
        C._lib.check(lib.sr_conv3x3_set_stamps(st.data_ptr()))
        run()
        torch.cuda.synchronize()
    finally:
        C._lib.check(lib.sr_conv3x3_set_stamps(None))
        C._lib.check(lib.sr_conv3x3_set_variant(0))
    s = st.view(nblk, 16).cpu()
    s = s[s[:, 1] > 0].double()
    if s.shape[0] == 0:
        sys.exit('no stamps: the library is not a -DSR_BAND_STAMPS build, or the call did not run the pph kernel')
    nt = s[:, 1]
    out = dict(variant=variant, shape=[B, H, W, cin, cout], blocks=int(s.shape[0]), tiles_per_block=float(nt.mean()),
               us_per_launch_unstamped=round(us, 2))
    last = torch.stack([s[i, 2 + 4 * (min(int(nt[i]), 3) - 1) + 3] for i in range(s.shape[0])])
    out['block_total'] = float((last - s[:, 0]).mean())
    tiles = []
    prev_end = s[:, 0]
    for ti in range(3):
        m = nt > ti
        if not bool(m.any()):
            break
        b = 2 + 4 * ti
        tiles.append(dict(blocks=int(m.sum()),
                          prologue=float((s[m, b] - prev_end[m]).mean()),  # entry / previous tile's end -> K loop
                          k_loop=float((s[m, b + 1] - s[m, b]).mean()),
                          epilogue_half0=float((s[m, b + 2] - s[m, b + 1]).mean()),
                          epilogue_half1=float((s[m, b + 3] - s[m, b + 2]).mean())))
        prev_end = s[:, b + 3]
    out['tiles'] = tiles
    if float(s[:, 14].sum()) > 0:
        out['operand_wait_per_tile'] = float((s[:, 14] / nt.clamp(max=3)).mean())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
