//! image_hash_hip.rs -- the hashing `split_segment` (emulator/src/state.rs:1477-1530) does between two segments, by libzkmhip.so
//! (zkm_image_hash, include/zkm_hip.h) instead of on one CPU thread: `Memory::update_page_hash` and `Memory::compute_image_id`
//! (emulator/src/memory.rs:415-471) in one device call.  The dirty pages are `wtrace[0]`; the hash pages the memory holds already go
//! in as `known`; the call returns the hash pages as the emulator would leave them (the caller writes them back into `pages`, or keeps
//! them on the device and hands them to the next split as `known`), `page_hash_root` and `image_id`.
//!
//! Goes into the zkm-emulator crate as `emulator/src/image_hash_hip.rs`; `wtrace` is private to `Memory`, so the call site is a method
//! of `Memory` that passes `&self.wtrace[0]`.  The reference items used here are checked by tests/test_rust_image_hash_names.py.
//! NOT COMPILED in the build image (no cargo / rustc there).
use std::cell::RefCell;
use std::collections::BTreeMap;
use std::os::raw::c_char;
use std::rc::Rc;

use anyhow::{ensure, Result};
use plonky2::hip::sys::*;

use crate::page::{CachedPage, PAGE_SIZE};

pub const PAGE_WORDS: usize = PAGE_SIZE / 4;
/// compute_image_id's root page (memory.rs:440)
pub const ROOT_PAGE_INDEX: u32 = 0x81020;

/// What `split_segment` needs from the two calls it replaces.
pub struct SplitHashes {
    /// the hash pages `update_page_hash` wrote, ascending: L1 pages, L2 pages, the root (zkm_image_hash_plan)
    pub plan: Vec<u32>,
    /// plan.len() x 1024 LE words: the pages as the emulator leaves them, the root page with the registers in it
    pub hash_words: Vec<u32>,
    pub page_hash_root: [u8; 32],
    pub image_id: [u8; 32],
}

/// The ascending hash pages that hashing these ascending dirty pages writes.
pub fn image_hash_plan(dirty_index: &[u32]) -> Vec<u32> {
    let n = unsafe { zkm_image_hash_plan(dirty_index.as_ptr(), dirty_index.len(), std::ptr::null_mut(), 0) };
    let mut plan = vec![0u32; n];
    unsafe { zkm_image_hash_plan(dirty_index.as_ptr(), dirty_index.len(), plan.as_mut_ptr(), n) };
    plan
}

fn page_words(page: &CachedPage, out: &mut Vec<u32>) {
    out.extend(page.data.chunks_exact(4).map(|b| u32::from_le_bytes([b[0], b[1], b[2], b[3]])));
}

/// `dirty`: `wtrace[0]` of the memory.  `pages`: the memory's page map, from which the plan's hash pages that exist already are taken.
/// `registers`: `get_registers_bytes()`.  One host wait.
pub fn split_hashes_hip(ctx: *mut zkm_ctx, dirty: &BTreeMap<u32, Rc<RefCell<CachedPage>>>, pages: &BTreeMap<u32, Rc<RefCell<CachedPage>>>,
                        pc: u32, registers: &[u8; 39 * 4]) -> Result<SplitHashes> {
    let dirty_index: Vec<u32> = dirty.keys().copied().collect();
    let mut dirty_words = Vec::with_capacity(dirty_index.len() * PAGE_WORDS);
    for page in dirty.values() {
        page_words(&page.borrow(), &mut dirty_words);
    }
    let plan = image_hash_plan(&dirty_index);
    ensure!(plan.last() == Some(&ROOT_PAGE_INDEX), "the plan does not end with the root page");
    let (mut known_index, mut known_words) = (Vec::new(), Vec::new());
    for q in &plan {
        if let Some(page) = pages.get(q) {
            known_index.push(*q);
            page_words(&page.borrow(), &mut known_words);
        }
    }
    let input = zkm_image_pages {
        dirty_index: dirty_index.as_ptr(), ndirty: dirty_index.len(), dirty_words: dirty_words.as_ptr(),
        known_index: known_index.as_ptr(), nknown: known_index.len(), known_words: known_words.as_ptr(),
        pc, registers: *registers,
    };
    let mut out = SplitHashes { hash_words: vec![0u32; plan.len() * PAGE_WORDS], plan, page_hash_root: [0; 32], image_id: [0; 32] };
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc = unsafe { zkm_image_hash(ctx, &input, out.hash_words.as_mut_ptr(), out.page_hash_root.as_mut_ptr(), out.image_id.as_mut_ptr(), &mut err) };
    check(rc, err)?;
    Ok(out)
}

/// The same result written back into the memory's page map, as `update_page_hash` and `compute_image_id` leave it.
pub fn store_hash_pages(pages: &mut BTreeMap<u32, Rc<RefCell<CachedPage>>>, hashes: &SplitHashes) {
    for (q, words) in hashes.plan.iter().zip(hashes.hash_words.chunks_exact(PAGE_WORDS)) {
        let page = pages.entry(*q).or_insert_with(|| Rc::new(RefCell::new(CachedPage::new())));
        for (dst, w) in page.borrow_mut().data.chunks_exact_mut(4).zip(words) {
            dst.copy_from_slice(&w.to_le_bytes());
        }
    }
}
