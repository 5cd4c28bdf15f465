"""Does the image kernel of buffer k+1 start before shift_iir of buffer k ends, on another queue?

    tools/trace_next_image.py KERNEL_TRACE.csv [--image SUBSTR] [--tail SUBSTR]

KERNEL_TRACE.csv: a `rocprofv3 --kernel-trace` table (columns Start_Timestamp, End_Timestamp, Kernel_Name, Queue_Id; times in ns).
An image launch counts for a shift_iir launch when it is running at the moment that launch ends -- it began before the end and
finishes after it -- whatever its length."""
import argparse
import csv


def summarise(rows, image, tail):
    ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "")) for r in rows)
    img = [k for k in ks if image in k[2]]
    iir = [k for k in ks if tail in k[2]]
    under = sum(any(s < e and end > e and q != qt for s, end, _, q in img) for _, e, _, qt in iir)
    return len(iir), under, sorted({k[3] for k in img}), sorted({k[3] for k in iir})


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("trace")
    ap.add_argument("--image", default="k_raster_fast", help="substring of the image kernel's name")
    ap.add_argument("--tail", default="k_shift_iir", help="substring of the name of the tail's last kernel")
    a = ap.parse_args()
    with open(a.trace, newline="") as f:
        n, under, qi, qt = summarise(list(csv.DictReader(f)), a.image, a.tail)
    print(f"shift_iir launches: {n}; with the next buffer's image kernel already running on another queue when they end: {under}")
    print("queues: image", qi, "shift_iir", qt)


if __name__ == "__main__":
    main()
