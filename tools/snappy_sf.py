"""Snappy Parquet decode at a given scale factor: best of 3, device vs pyarrow (host); every column is compared with the table that was written.  usage: snappy_sf.py SF"""
import io, json, os, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import pyarrow as pa
import pyarrow.parquet as pq
import arrow_ballista_amd as g
import tpch_util as T
from arrow_ballista_amd import scan
sf = int(sys.argv[1])
tc = g.TaskContext(device=0)
n = T.LINEITEM_ROWS.get(sf, 6_000_000 * sf)
li = T.lineitem_host_to_arrow(T.gen_lineitem_host(n), n)
li = li.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in li.schema]))
buf = io.BytesIO()
pq.write_table(li, buf, compression="SNAPPY", use_dictionary=True, data_page_size=1 << 20, row_group_size=1 << 20)
sfile = buf.getvalue()
del buf
best = None
for _ in range(3):
    tc.sync(); t0 = time.perf_counter(); r = scan.read_parquet(tc, sfile); tc.sync(); dt = time.perf_counter() - t0
    best = dt if best is None or dt < best else best
rows = r.num_rows
got = r.to_arrow(tc.ctx)
del r                                   # the device table goes before the comparison: at SF10 the host copies are large enough
unequal = [name for name in li.schema.names if not got.column(name).equals(li.column(name))]
ok = got.schema.names == li.schema.names and not unequal
del got
# the host baseline reads an Arrow-owned copy of the file: a buffer that wraps the Python bytes takes the GIL when it is released, and the
# last owner can be one of Arrow's reader threads while the interpreter is already finalising ("terminate called without an active exception")
abuf = pa.allocate_buffer(len(sfile)); memoryview(abuf).cast('B')[:] = sfile
t0 = time.perf_counter(); pq.read_table(pa.BufferReader(abuf)); host = time.perf_counter() - t0
print(json.dumps({"sf": sf, "rows": rows, "file_bytes": len(sfile), "device_ms": best * 1e3, "rows_per_s": rows / best, "pyarrow_host_ms": host * 1e3, "pj": os.environ.get("GPUQ_SNAPPY_PJ", "1"), "columns_equal": ok, "unequal": unequal}))
