//! check_ctls_hip.rs -- testutils::check_ctls (cross_table_lookup.rs:1486-1581) on the GPU: zkm_check_ctls of libzkmhip.so
//! (include/zkm_hip.h) behind the reference's argument list, panicking with the reference's message.
//!
//! The fields of Column, Filter and TableWithColumns are private to `cross_table_lookup`, so this file goes into the zkm-prover crate
//! as a CHILD of that module -- `prover/src/cross_table_lookup/check_ctls_hip.rs`, declared in cross_table_lookup.rs as
//!
//!     #[cfg(feature = "hip")] pub(crate) mod check_ctls_hip;
//!
//! -- and prove_with_traces (prover.rs:171-176) calls `check_ctls_hip(ctx, &trace_poly_values, &all_stark.cross_table_lookups)` where
//! it calls `check_ctls` under the `test` feature.  For tables that are already on the device (zkm_segment_tables) use
//! `segment_check_ctls_hip` on the staged block's pointers.  The reference items used here are checked by
//! tests/test_rust_check_ctls_names.py.  NOT COMPILED in the build image (no cargo / rustc there).
use std::ffi::CStr;
use std::os::raw::c_char;

use plonky2::field::polynomial::PolynomialValues;
use plonky2::field::types::PrimeField64;
use plonky2::hip::sys::*;

use super::{Column, CrossTableLookup, Filter, TableWithColumns};
use crate::all_stark::Table;
use crate::prove_hip::zkm_table_id;

/// The column sets of one table as zkm_ctl_table takes them (the arrays a zkm_ctl_table points into).
#[derive(Default)]
struct TableDesc {
    columns: Vec<zkm_column>,
    term_col: Vec<u32>,
    term_coeff: Vec<u64>,
    colsets: Vec<zkm_colset>,
    filter_idx: Vec<u32>,
}

impl TableDesc {
    fn column<F: PrimeField64>(&mut self, c: &Column<F>) -> u32 {
        let term_off = self.term_col.len() as u32;
        for (col, coeff) in c.linear_combination.iter().chain(c.next_row_linear_combination.iter()) {
            self.term_col.push(*col as u32);
            self.term_coeff.push(coeff.to_canonical_u64());
        }
        self.columns.push(zkm_column { n_local: c.linear_combination.len() as u32, n_next: c.next_row_linear_combination.len() as u32,
                                       term_off, _pad: 0, constant: c.constant.to_canonical_u64() });
        self.columns.len() as u32 - 1
    }

    /// TableWithColumns -> a column set: its columns as one consecutive range, then the filter's columns.
    fn colset<F: PrimeField64>(&mut self, t: &TableWithColumns<F>) -> u32 {
        let col_off = self.columns.len() as u32;
        for c in &t.columns {
            self.column(c);
        }
        let mut set = zkm_colset { ncols: t.columns.len() as u32, col_off, ..Default::default() };
        if let Some(Filter { products, constants }) = &t.filter {
            set.has_filter = 1;
            let prods: Vec<(u32, u32)> = products.iter().map(|(a, b)| (self.column(a), self.column(b))).collect();
            let consts: Vec<u32> = constants.iter().map(|c| self.column(c)).collect();
            set.nprod = prods.len() as u32;
            set.prod_off = self.filter_idx.len() as u32;
            for (a, b) in prods {
                self.filter_idx.extend([a, b]);
            }
            set.nconst = consts.len() as u32;
            set.const_off = self.filter_idx.len() as u32;
            self.filter_idx.extend(consts);
        }
        self.colsets.push(set);
        self.colsets.len() as u32 - 1
    }

    fn raw(&self) -> zkm_ctl_table {
        zkm_ctl_table { columns: self.columns.as_ptr(), ncolumns: self.columns.len(), term_col: self.term_col.as_ptr(),
                        term_coeff: self.term_coeff.as_ptr(), nterms: self.term_col.len(), colsets: self.colsets.as_ptr(),
                        ncolsets: self.colsets.len(), filter_idx: self.filter_idx.as_ptr(), nfilter_idx: self.filter_idx.len() }
    }
}

fn empty_report() -> zkm_ctl_report {
    // (plain integers: all-zero is a valid value)
    unsafe { std::mem::zeroed() }
}

fn finish(rc: i32, err: *mut c_char, report: &zkm_ctl_report) {
    if rc == 0 {
        return;
    }
    let msg = if err.is_null() { format!("check_ctls: error {rc}") } else { unsafe { CStr::from_ptr(err) }.to_string_lossy().into_owned() };
    // (the message is malloc'd by the library; a panic is the end of a debug run, so it is not released)
    panic!("{msg} (kind {}, attempts {})", report.kind, report.attempts);
}

/// `check_ctls(trace_poly_values, cross_table_lookups)` (cross_table_lookup.rs:1496-1503) on the GPU of `ctx`: panics with
/// "CTL #i: Row [..] is present a times in the looking tables, but b times in the looked table. ..." or "Non-binary filter?" as the
/// reference does (:1560, :1572-1579).  Tables are named by their position in `trace_poly_values` (the Table enum, all_stark.rs:96-110).
pub fn check_ctls_hip<F: PrimeField64>(ctx: *mut zkm_ctx, trace_poly_values: &[Vec<PolynomialValues<F>>], cross_table_lookups: &[CrossTableLookup<F>]) {
    let mut descs: Vec<TableDesc> = trace_poly_values.iter().map(|_| TableDesc::default()).collect();
    let mut sides: Vec<zkm_ctl_side> = Vec::new();
    let mut ctls: Vec<zkm_cross_table_lookup> = Vec::new();
    for ctl in cross_table_lookups {
        let looking_off = sides.len() as u32;
        for t in &ctl.looking_tables {
            let table = t.table as u32;
            sides.push(zkm_ctl_side { table, colset: descs[table as usize].colset(t) });
        }
        let table = ctl.looked_table.table as u32;
        let looked = zkm_ctl_side { table, colset: descs[table as usize].colset(&ctl.looked_table) };
        ctls.push(zkm_cross_table_lookup { nlooking: ctl.looking_tables.len() as u32, looking_off, looked });
    }
    let raws: Vec<zkm_ctl_table> = descs.iter().map(|d| d.raw()).collect();
    // one pointer per column: Vec<PolynomialValues<F>> as it is (F = GoldilocksField is a transparent u64)
    let columns: Vec<Vec<*const u64>> = trace_poly_values.iter().map(|t| t.iter().map(|p| p.values.as_ptr() as *const u64).collect()).collect();
    let tables: Vec<zkm_table_input> = trace_poly_values.iter().enumerate().map(|(i, t)| zkm_table_input {
        table_id: zkm_table_id(Table::all()[i]),   // (names the table in messages)
        trace: std::ptr::null(), ncols: t.len(), log_n: t[0].len().trailing_zeros(), ctl: &raws[i], columns: columns[i].as_ptr() }).collect();
    let mut report = empty_report();
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc = unsafe { zkm_check_ctls(ctx, tables.as_ptr(), tables.len(), ctls.as_ptr(), sides.as_ptr(), ctls.len(), &mut report, &mut err) };
    finish(rc, err, &report);
}

/// The same for the AllStark inside the library on twelve device-resident tables (Table::all() order), e.g. `DeviceSegment::tables()`
/// of segment_hip.rs: nothing is downloaded.
pub fn segment_check_ctls_hip(ctx: *mut zkm_ctx, traces: &[*const u64; 12], log_n: &[u32; 12]) {
    let mut report = empty_report();
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc = unsafe { zkm_segment_check_ctls(ctx, traces.as_ptr(), log_n.as_ptr(), &mut report, &mut err) };
    finish(rc, err, &report);
}
